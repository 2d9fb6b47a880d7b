// Stand-alone AddressSanitizer / UBSan run of the gain-fusion per-value code (csrc/heat.h through
// rpt_heat_host and rpt_fixed4_repr, csrc/heat.cpp -- what k_seg_p99, k_heat and the
// RPT_TEXT_PLY4 kernels run per value), through exactly sized heap buffers so that a byte written
// past an array is seen.
//
//   rpt_heat_host    segments of 1, 2, 11, 26, 31, 52, 101, 255..257 and 5000 values with empty
//                    ones between (both lerp branches, an integer rank), of echoes with ties, one
//                    value, mixed signs and values above p99; checks min and p99 against a sort,
//                    z inside 0..255 and the colour at the ends of the four pieces; colours-only
//                    over every piece boundary and its float neighbours; bad offsets -> RPT_EINVAL
//   rpt_fixed4_repr  every biased exponent, both signs, fixed and random mantissas, the ties
//                    0.03125 / 0.09375, -0.00001, the carry 9999.99995, -0.0, 2^39, 2^40, NaN,
//                    inf: length, NULs, and the text against snprintf("%.4f")
//
//   make -C tools/asan heat
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "heat.h"
#include "rpt.h"

static uint64_t next_u64(uint64_t* s) {  // splitmix64
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <class T>
static T* heap(size_t n) {  // exactly sized: the redzone sits right behind the last element
  return static_cast<T*>(std::malloc(sizeof(T) * (n ? n : 1)));
}

static int64_t check_heat() {
  const int sizes[] = {1, 0, 2, 11, 26, 0, 31, 52, 101, 255, 256, 257, 0, 5000, 0};
  const int S = (int)(sizeof(sizes) / sizeof(sizes[0]));
  int64_t bad = 0;
  uint64_t seed = 1414;
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<int64_t> off(1, 0);
    for (int s = 0; s < S; ++s) off.push_back(off.back() + sizes[s]);
    const int64_t n = off.back();
    float* v = heap<float>((size_t)n);
    int64_t* o = heap<int64_t>((size_t)S + 1);
    float* mn = heap<float>((size_t)S);
    float* p = heap<float>((size_t)S);
    float* z = heap<float>((size_t)n);
    uint8_t* rgb = heap<uint8_t>((size_t)n * 3);
    std::memcpy(o, off.data(), sizeof(int64_t) * (S + 1));
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t r = next_u64(&seed);
      if (kind == 0) v[i] = (float)(6 + r % 250);                       // echoes, ties
      else if (kind == 1) v[i] = 100.0f;                                // p99 <= min
      else if (kind == 2) v[i] = ((float)(r % 2000001) - 1.0e6f) / 1024.0f;  // mixed signs
      else v[i] = (r % 50 == 0) ? 65536.5f : (float)(6 + r % 30);       // far above the rank
    }
    if (rpt_heat_host(v, n, o, S, 0, mn, p, z, rgb) != RPT_OK) ++bad;
    for (int s = 0; s < S; ++s) {
      const int64_t a = off[s], m = off[s + 1] - a;
      if (m == 0) continue;
      std::vector<float> srt(v + a, v + a + m);
      std::sort(srt.begin(), srt.end());
      int64_t lo, hi;
      float t;
      rpt::heat::rank99(m, &lo, &hi, &t);
      const float want = rpt::heat::lerp99(srt[(size_t)lo], srt[(size_t)hi], t);
      if (mn[s] != srt[0] || std::memcmp(&want, p + s, 4) != 0) ++bad;
      if (lo < 0 || hi >= m || hi < lo || !(t >= 0.0f && t < 1.0f)) ++bad;
      for (int64_t i = a; i < a + m; ++i) {
        if (!(z[i] >= 0.0f && z[i] <= 255.0f)) ++bad;
        if (p[s] <= mn[s] && (z[i] != 0.0f || rgb[3 * i] != 0 || rgb[3 * i + 2] != 255)) ++bad;
        if (v[i] == mn[s] && (rgb[3 * i] != 0 || rgb[3 * i + 1] != 0 || rgb[3 * i + 2] != 255))
          ++bad;
        if (p[s] > mn[s] && v[i] >= p[s] &&
            (z[i] != 255.0f || rgb[3 * i] != 255 || rgb[3 * i + 1] != 0 || rgb[3 * i + 2] != 0))
          ++bad;
      }
    }
    // offsets that are not this array's
    o[S] = n + 1;
    if (rpt_heat_host(v, n, o, S, 0, mn, p, z, rgb) != RPT_EINVAL) ++bad;
    o[S] = n;
    o[1] = -1;
    if (rpt_heat_host(v, n, o, S, 0, mn, p, z, rgb) != RPT_EINVAL) ++bad;
    // outputs that are not wanted
    o[1] = off[1];
    if (rpt_heat_host(v, n, o, S, 0, nullptr, nullptr, nullptr, nullptr) != RPT_OK) ++bad;
    std::free(v);
    std::free(o);
    std::free(mn);
    std::free(p);
    std::free(z);
    std::free(rgb);
  }
  // colours only: the piece boundaries, their float neighbours, the ends
  const float edges[] = {0.0f, 63.75f, 127.5f, 191.25f, 255.0f};
  const uint8_t at[5][3] = {{0, 0, 255}, {0, 255, 255}, {0, 255, 0}, {255, 255, 0}, {255, 0, 0}};
  const int64_t n = 15;
  float* zv = heap<float>(n);
  uint8_t* c = heap<uint8_t>(n * 3);
  for (int k = 0; k < 5; ++k) {
    zv[3 * k] = edges[k];
    zv[3 * k + 1] = k ? std::nextafterf(edges[k], -1.0f) : 0.0f;
    zv[3 * k + 2] = k < 4 ? std::nextafterf(edges[k], 999.0f) : 255.0f;
  }
  if (rpt_heat_host(zv, n, nullptr, 0, 1, nullptr, nullptr, nullptr, c) != RPT_OK) ++bad;
  for (int k = 0; k < 5; ++k) {
    if (std::memcmp(c + 9 * k, at[k], 3) != 0) ++bad;
    for (int j = 1; j < 3; ++j)  // a neighbour's colour is within one count of the boundary's
      for (int ch = 0; ch < 3; ++ch)
        if (std::abs((int)c[9 * k + 3 * j + ch] - (int)at[k][ch]) > 1) ++bad;
  }
  std::free(zv);
  std::free(c);
  if (rpt_heat_host(nullptr, 0, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr) != RPT_OK ||
      rpt_heat_host(nullptr, 1, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr) != RPT_EINVAL)
    ++bad;
  return bad;
}

static int64_t check_fixed4(int* longest_out, int64_t* n_out) {
  const uint32_t fixed[] = {0u, 1u, 2u, 0x400000u, 0x7ffffeu, 0x7fffffu};
  const float named_f[] = {0.03125f, 0.09375f, -0.00001f, 9999.99995f, -0.0f, 0.0f,
                           549755813888.0f, -549755813888.0f, 1099511627776.0f, 0.00005f,
                           0.00015f, 0.99995f, 1.5f, 255.0f, 63.75f};
  const char* named_s[] = {"0.0312", "0.0938", "-0.0000", "10000.0000", "-0.0000", "0.0000",
                           "549755813888.0000", "-549755813888.0000", ""};
  std::vector<uint32_t> bits;
  for (float f : named_f) bits.push_back(rpt::heat::f2u(f));
  const uint32_t special[] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffffffffu, 0x00000001u,
                              0x807fffffu, 0x00800000u};
  for (uint32_t b : special) bits.push_back(b);
  uint64_t seed = 1415;
  for (uint32_t e = 0; e < 256; ++e)
    for (uint32_t sign = 0; sign < 2; ++sign) {
      for (uint32_t m : fixed) bits.push_back((sign << 31) | (e << 23) | m);
      for (int k = 0; k < 200; ++k)
        bits.push_back((sign << 31) | (e << 23) | (uint32_t)(next_u64(&seed) & 0x7fffffu));
    }
  const int64_t n = (int64_t)bits.size();
  float* v = heap<float>((size_t)n);
  char* out = heap<char>((size_t)RPT_FIXED4_SLOT * n);
  int32_t* len = heap<int32_t>((size_t)n);
  std::memcpy(v, bits.data(), sizeof(float) * n);
  int64_t bad = 0;
  if (rpt_fixed4_repr(v, n, out, len) != RPT_OK) ++bad;
  int longest = 0;
  for (int64_t i = 0; i < n; ++i) {
    const char* s = out + i * RPT_FIXED4_SLOT;
    const uint32_t e = (bits[i] >> 23) & 0xffu;
    bool ok;
    if (e >= 127u + 40u) {  // NaN, inf, |v| >= 2^40
      ok = len[i] == 0;
      for (int k = 0; k < RPT_FIXED4_SLOT; ++k) ok = ok && s[k] == 0;
    } else {
      char want[64];
      const int wl = std::snprintf(want, sizeof(want), "%.4f", (double)v[i]);
      ok = len[i] == wl && wl <= 19 && std::memcmp(s, want, (size_t)wl) == 0;
      for (int k = len[i] > 0 ? len[i] : 0; ok && k < RPT_FIXED4_SLOT; ++k) ok = s[k] == 0;
      if (len[i] > longest) longest = len[i];
    }
    if (i < 9 && std::strcmp(s, named_s[i]) != 0) ok = false;
    if (!ok && bad++ < 10)
      std::fprintf(stderr, "heat_main: bits 0x%08x -> len %d \"%.20s\"\n", bits[i], len[i], s);
  }
  std::free(v);
  std::free(out);
  std::free(len);
  if (rpt_fixed4_repr(nullptr, 0, nullptr, nullptr) != RPT_OK ||
      rpt_fixed4_repr(nullptr, 1, nullptr, nullptr) != RPT_EINVAL)
    ++bad;
  *longest_out = longest;
  *n_out = n;
  return bad;
}

int main() {
  const int64_t bad_heat = check_heat();
  int longest = 0;
  int64_t n = 0;
  const int64_t bad_fixed = check_fixed4(&longest, &n);
  std::printf("heat_main: heat %lld bad; fixed4 %lld values, longest text %d, %lld bad\n",
              (long long)bad_heat, (long long)n, longest, (long long)bad_fixed);
  return bad_heat == 0 && bad_fixed == 0 && longest == 19 ? 0 : 1;
}
