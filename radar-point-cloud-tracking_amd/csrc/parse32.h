// A plain decimal token -> float32, as np.float32(float(token)) gives it: CPython's correctly
// rounded string-to-double conversion followed by the round-to-nearest-even cast to float32 (two
// roundings: "5.73106837272644" reads 5.7310686111450195, not the 5.731068134307861 a direct
// rounding to float32 would give).  One routine for the device (csrc/ply_parse.hip, the vertex
// rows of load_ply) and the host (rpt_decimal_parse_host in csrc/parse32.cpp).
//
// Domain: [+-]? followed by digits[.digits*] or .digits, nothing but the bytes 0-9 + - . ; with
// the leading zeros of the digit string removed,
//   at most 19 digits        m, the integer they form, fits the 64-bit accumulator
//   m <= 2^53                double(m) is exact
//   f <= 22                  f = digits behind the point; 10^f is exact in a double
// Then ONE IEEE float64 division double(m) / 10^f is the correctly rounded double (Clinger, "How
// to read floating point numbers accurately", PLDI 1990: the fast path; no division at f == 0),
// the sign goes onto the double ("-0.000000" is -0.0) and the float64 -> float32 conversion under
// the default rounding mode is the reference's cast.  The largest value is 2^53 and the smallest
// non-zero one 1e-22: neither overflow nor a float32 subnormal can occur.
//
// Everything else -- an exponent, nan, inf, '_', a second point, a sign alone, the empty token,
// any other byte, more digits -- is OUTSIDE the domain: parse() returns false and the caller hands
// the text to the host reader.  The division has to be the correctly rounded one (no fast-math,
// no reciprocal; rpt/_build.py compiles with -ffp-contract=off and without fast-math).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_P32_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RPT_P32_HD inline
#endif

namespace rpt {
namespace parse32 {

constexpr int kMaxDigits = 19;
constexpr int kMaxFraction = 22;
constexpr uint64_t kMaxMantissa = 1ull << 53;

RPT_P32_HD double pow10_exact(int f) {  // 0 <= f <= 22
  constexpr double t[kMaxFraction + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,
                                          1e8,  1e9,  1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                          1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[f];
}

// s[0..len) -> *out; false (and *out untouched) when the token is outside the domain.  Reads
// nothing but s[0..len).
RPT_P32_HD bool parse(const uint8_t* s, int len, float* out) {
  if (len <= 0) return false;
  int i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    i = 1;
  }
  uint64_t m = 0;
  int nd = 0;  // digits from the first non-zero one on
  int f = 0;   // digits behind the point
  bool any = false, point = false;
  for (; i < len; ++i) {
    const uint32_t c = s[i];
    if (c == '.') {
      if (point) return false;
      point = true;
      continue;
    }
    const uint32_t d = c - (uint32_t)'0';
    if (d > 9u) return false;
    any = true;
    if (point && ++f > kMaxFraction) return false;
    if (nd != 0 || d != 0u) {
      if (++nd > kMaxDigits) return false;
      m = m * 10u + d;  // < 10^19 < 2^64
    }
  }
  if (!any || m > kMaxMantissa) return false;
  double v = (double)m;
  if (f) v = v / pow10_exact(f);
  if (neg) v = -v;
  *out = (float)v;
  return true;
}

}  // namespace parse32
}  // namespace rpt
