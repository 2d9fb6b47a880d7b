// Stand-alone AddressSanitizer / UBSan run of the shortest-repr formatter (csrc/repr32.h through
// rpt_float32_repr, csrc/repr32.cpp -- the code the RPT_TEXT_XYZ_REPR kernels run per value):
// the strata of tests/_repr_pool.py (every biased exponent 0..254, both signs, the fixed
// mantissas and seeded random ones, the named bit patterns) plus NaN and inf, through exactly
// sized heap buffers so that a byte written past a slot is seen.  Checks: status, length 1..19,
// no NUL inside the text, NULs behind it, the text reads back as the value (strtof).
//
//   make -C tools/asan repr32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rpt.h"

static uint64_t next_u64(uint64_t* s) {  // splitmix64
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main() {
  const uint32_t fixed[] = {0u, 1u, 2u, 0x400000u, 0x7ffffeu, 0x7fffffu};
  const uint32_t named[] = {0x38d1b717u, 0x38d1b718u, 0x5a0e1bc9u, 0x5a0e1bcau, 0x5a0e1bcbu,
                            0x4c215b00u, 0x4dc912dau, 0x4cf8ca6cu, 0x4dda688cu, 0x4c470e82u,
                            0x00000000u, 0x80000000u, 0x00000001u, 0x007fffffu, 0x00800000u,
                            0x7f7fffffu, 0x3f800000u, 0x4b800000u, 0x3dcccccdu, 0x477fe080u,
                            0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffffffffu};
  const int kRandom = 500;
  std::vector<uint32_t> bits(named, named + sizeof(named) / sizeof(named[0]));
  uint64_t seed = 1310;
  for (uint32_t e = 0; e < 255; ++e) {
    for (uint32_t sign = 0; sign < 2; ++sign) {
      for (uint32_t m : fixed) bits.push_back((sign << 31) | (e << 23) | m);
      for (int k = 0; k < kRandom; ++k)
        bits.push_back((sign << 31) | (e << 23) | (uint32_t)(next_u64(&seed) & 0x7fffffu));
    }
  }
  const int64_t n = (int64_t)bits.size();
  // exactly sized heap blocks: the redzones sit right behind the last slot and the last length
  float* v = static_cast<float*>(std::malloc(sizeof(float) * n));
  char* out = static_cast<char*>(std::malloc((size_t)RPT_FLOAT32_REPR_SLOT * n));
  int32_t* len = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * n));
  if (!v || !out || !len) return 2;
  std::memcpy(v, bits.data(), sizeof(float) * n);
  if (rpt_float32_repr(v, n, out, len) != RPT_OK) {
    std::fprintf(stderr, "repr32_main: rpt_float32_repr failed\n");
    return 1;
  }
  int64_t bad = 0, outside = 0;
  int longest = 0;
  for (int64_t i = 0; i < n; ++i) {
    const char* s = out + i * RPT_FLOAT32_REPR_SLOT;
    const bool finite = ((bits[i] >> 23) & 0xffu) != 0xffu;
    bool ok;
    if (!finite) {
      ++outside;
      ok = len[i] == 0;
      for (int k = 0; k < RPT_FLOAT32_REPR_SLOT; ++k) ok = ok && s[k] == 0;
    } else {
      ok = len[i] >= 1 && len[i] <= 19;
      for (int k = 0; ok && k < RPT_FLOAT32_REPR_SLOT; ++k) ok = (k < len[i]) == (s[k] != 0);
      if (ok) {
        const float back = std::strtof(s, nullptr);  // NUL-terminated: len <= 19 < slot
        uint32_t b;
        std::memcpy(&b, &back, sizeof(b));
        ok = b == bits[i];
        if (len[i] > longest) longest = len[i];
      }
    }
    if (!ok && bad++ < 10)
      std::fprintf(stderr, "repr32_main: bits 0x%08x -> len %d \"%.20s\"\n", bits[i], len[i], s);
  }
  std::free(v);
  std::free(out);
  std::free(len);
  if (rpt_float32_repr(nullptr, 0, nullptr, nullptr) != RPT_OK ||
      rpt_float32_repr(nullptr, 1, nullptr, nullptr) != RPT_EINVAL)
    ++bad;
  std::printf("repr32_main: %lld values (%lld NaN/inf), longest text %d, %lld bad\n",
              (long long)n, (long long)outside, longest, (long long)bad);
  return bad == 0 && longest == 19 ? 0 : 1;
}
