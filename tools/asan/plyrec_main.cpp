// Stand-alone AddressSanitizer / UBSan run of the denoise PLY writer's per-value code
// (csrc/plyrec.h through rpt_ply_records_host, csrc/plyrec.cpp -- what k_ply_count, k_ply_write and
// k_ply_colors run per point), through exactly sized heap buffers so that a byte written past an
// array is seen.
//
//   viridis_index   0, -0.0, 255 and its float neighbours, negatives, values above 255, every
//                   k * 255 / 256 with both float32 neighbours, +-inf, NaN: the row against the
//                   rule evaluated in double (exact for these operands up to the division's
//                   rounding, which is done in float32 here as there)
//   records         a LUT that stores its row number, so that a record's colour names the row
//                   taken: labels -1, 0, 19, 20, 39, 2^31 - 1, -7 and INT32_MIN, both colour
//                   modes, signal_only on and off; coordinates with NaN payloads, -0.0, inf and a
//                   subnormal copied bit for bit; the kept count and the largest label
//   limits          n = 0, count only (out NULL), out one byte too small, signal_only without
//                   labels, n = 2^31
//
//   make -C tools/asan plyrec
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "plyrec.h"
#include "rpt.h"

template <class T>
static T* heap(size_t n) {  // exactly sized: the redzone sits right behind the last element
  return static_cast<T*>(std::malloc(sizeof(T) * (n ? n : 1)));
}

static std::vector<float> edge_values() {
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> v = {0.0f, -0.0f, 255.0f, 254.99998f, 255.00002f, -1.0f, -0.5f, -1e-30f,
                          -300.0f, 256.0f, 300.0f, 1e10f, inf, -inf,
                          std::numeric_limits<float>::quiet_NaN()};
  for (int k = 0; k <= 256; ++k) {
    const float e = (float)((double)k * 255.0 / 256.0);
    v.push_back(e);
    v.push_back(std::nextafterf(e, -1e9f));
    v.push_back(std::nextafterf(e, 1e9f));
  }
  return v;
}

static int want_row(float z) {
  if (std::isnan(z)) return 256;
  float zn = z / 255.0f;
  zn = std::fmax(zn, 0.0f);
  zn = std::fmin(zn, 1.0f);
  const double f = (double)zn * 256.0;
  return f == 256.0 ? 255 : (int)f;
}

int main() {
  namespace pr = rpt::plyrec;
  int64_t bad = 0;
  const std::vector<float> edges = edge_values();
  for (float z : edges)
    if (pr::viridis_index(z) != want_row(z)) ++bad;
  if (pr::viridis_index(0.0f) != 0 || pr::viridis_index(-0.0f) != 0 ||
      pr::viridis_index(255.0f) != 255 || pr::viridis_index(1e10f) != 255 ||
      pr::viridis_index(-300.0f) != 0)
    ++bad;

  // a LUT whose row r holds (r & 255, r >> 8, 7)
  uint8_t* lutv = heap<uint8_t>(257 * 3);
  uint8_t* lut20 = heap<uint8_t>(20 * 3);
  for (int r = 0; r < 257; ++r) {
    lutv[3 * r] = (uint8_t)(r & 255);
    lutv[3 * r + 1] = (uint8_t)(r >> 8);
    lutv[3 * r + 2] = 7;
  }
  for (int r = 0; r < 20; ++r) {
    lut20[3 * r] = (uint8_t)r;
    lut20[3 * r + 1] = 0;
    lut20[3 * r + 2] = 7;
  }
  const int32_t named[] = {-1, 0, 19, 20, 39, 2147483647, -7, (-2147483647 - 1)};
  const uint32_t odd_bits[] = {0x7fc12345u, 0xffc00001u, 0x80000000u, 0x7f800000u, 0x00000001u};
  const int64_t n = (int64_t)edges.size();
  float* x = heap<float>((size_t)n);
  float* y = heap<float>((size_t)n);
  float* z = heap<float>((size_t)n);
  int32_t* lab = heap<int32_t>((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t b = i < 5 ? odd_bits[i] : 0x3f800000u + (uint32_t)i * 977u;
    std::memcpy(x + i, &b, 4);
    const uint32_t c = ~b & 0xff7fffffu;
    std::memcpy(y + i, &c, 4);
    z[i] = edges[(size_t)i];
    lab[i] = i < 64 ? named[i % 8] : (int32_t)((i * 37) % 61) - 1;
  }
  for (int mode = 0; mode < 3; ++mode) {  // plain; labels, all points; labels, signal only
    const int32_t* l = mode ? lab : nullptr;
    const int32_t so = mode == 2;
    const uint8_t* lut = mode ? lut20 : lutv;
    int32_t mx = 12345;
    const int64_t kept = rpt_ply_records_host(x, y, z, l, so, lut, n, nullptr, 0, &mx);
    int64_t want_kept = 0;
    for (int64_t i = 0; i < n; ++i) want_kept += !so || lab[i] >= 0;
    if (kept != want_kept || mx != (mode ? 2147483647 : -1)) ++bad;
    uint8_t* out = heap<uint8_t>((size_t)kept * 15);
    if (rpt_ply_records_host(x, y, z, l, so, lut, n, out, kept * 15, nullptr) != kept) ++bad;
    if (kept > 0 && rpt_ply_records_host(x, y, z, l, so, lut, n, out, kept * 15 - 1, nullptr) !=
                        -RPT_EINVAL)
      ++bad;
    int64_t r = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (so && lab[i] < 0) continue;
      const uint8_t* p = out + 15 * r++;
      if (std::memcmp(p, x + i, 4) || std::memcmp(p + 4, y + i, 4) || std::memcmp(p + 8, z + i, 4))
        ++bad;
      if (!mode) {
        const int row = want_row(z[i]);
        if (p[12] != (row & 255) || p[13] != (row >> 8) || p[14] != 7) ++bad;
      } else if (lab[i] < 0) {
        if (p[12] != 128 || p[13] != 128 || p[14] != 128) ++bad;
      } else {
        if (p[12] != lab[i] % 20 || p[13] != 0 || p[14] != 7) ++bad;
      }
    }
    if (r != kept) ++bad;
    std::free(out);
  }
  // limits
  if (rpt_ply_records_host(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0,
                           nullptr) != 0)
    ++bad;
  if (rpt_ply_records_host(x, y, z, nullptr, 1, lutv, n, nullptr, 0, nullptr) != -RPT_EINVAL)
    ++bad;
  if (rpt_ply_records_host(x, y, z, nullptr, 0, lutv, -1, nullptr, 0, nullptr) != -RPT_EINVAL)
    ++bad;
  if (rpt_ply_records_host(nullptr, nullptr, nullptr, nullptr, 0, nullptr, int64_t(1) << 31,
                           nullptr, 0, nullptr) != -RPT_ENOTSUP)
    ++bad;
  if (rpt_ply_record_tiles(0) != 0 || rpt_ply_record_tiles(1) != 1 ||
      rpt_ply_record_tiles(pr::kTile) != 1 || rpt_ply_record_tiles(pr::kTile + 1) != 2)
    ++bad;
  std::free(x);
  std::free(y);
  std::free(z);
  std::free(lab);
  std::free(lutv);
  std::free(lut20);
  std::printf("plyrec_main: %lld values, %lld bad\n", (long long)n, (long long)bad);
  return bad == 0 ? 0 : 1;
}
