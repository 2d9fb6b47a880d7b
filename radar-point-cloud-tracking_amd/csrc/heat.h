// Per-value code of the gain-fusion PLY builder (PointCloudWork/5_gain_fusion_ply_builder.py),
// one routine each for the device (csrc/fusion_color.hip, csrc/text.hip layout RPT_TEXT_PLY4) and
// the host (rpt_heat_host / rpt_fixed4_repr in csrc/heat.cpp, tools/asan/heat_main.cpp):
//
//   heat::key / unkey      order-preserving uint32 image of a float32 (radix select, minimum)
//   heat::rank99           the two order statistics np.percentile(a, 99) reads and their weight
//   heat::lerp99           numpy's _lerp between them
//   heat::normalize        normalize_intensity :276-289 for one value given its segment's
//                          minimum and 99th percentile
//   heat::rgb              intensity_to_rgb :292-327, the four-piece heat map
//   fixed4::decimal/length/put   "%.4f" % float(np.float32(v)) in integers
//
// Every float operation is a single float32 operation rounded once (the build's global
// -ffp-contract=off keeps FMA out; divisions are IEEE divisions), which is what numpy does on
// float32 arrays.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_HEAT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RPT_HEAT_HD inline
#endif

namespace rpt {
namespace heat {

RPT_HEAT_HD uint32_t f2u(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return u;
}
RPT_HEAT_HD float u2f(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof(f));
  return f;
}

// IEEE float32 division, correctly rounded on both sides
RPT_HEAT_HD float fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// a < b  <=>  key(a) < key(b) for every pair of non-NaN floats (-0.0 sorts below +0.0)
RPT_HEAT_HD uint32_t key(float f) {
  const uint32_t u = f2u(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RPT_HEAT_HD float unkey(uint32_t k) {
  return u2f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// np.percentile(a, 99) of n >= 1 float32 values (method "linear"): the virtual index
// float32(n - 1) * (float32(99) / float32(100)) as a float32 product, its floor lo, the next index
// hi (clamped to n - 1) and the weight t = vi - lo (exact).
RPT_HEAT_HD void rank99(int64_t n, int64_t* lo, int64_t* hi, float* t) {
  const float q = 99.0f / 100.0f;
  const float vi = (float)(n - 1) * q;
  int64_t l = (int64_t)vi;  // vi >= 0: truncation is floor
  if (l > n - 1) l = n - 1;
  *lo = l;
  *hi = l + 1 < n ? l + 1 : n - 1;
  *t = vi - (float)l;
}

// numpy's _lerp(a, b, t): a + (b - a) * t below one half, b - (b - a) * (1 - t) from there on
RPT_HEAT_HD float lerp99(float a, float b, float t) {
  const float d = b - a;
  if (t < 0.5f) {
    const float dt = d * t;
    return a + dt;
  }
  const float u = 1.0f - t;
  const float du = d * u;
  return b - du;
}

// clip((v - mn) / (p99 - mn) * 255.0, 0, 255); 0 for a segment with p99 <= mn
RPT_HEAT_HD float normalize(float v, float mn, float p99) {
  if (p99 <= mn) return 0.0f;
  const float num = v - mn;
  const float den = p99 - mn;
  const float r = fdiv(num, den);
  float z = r * 255.0f;
  if (z < 0.0f) z = 0.0f;     // np.clip: minimum(maximum(z, 0), 255)
  if (z > 255.0f) z = 255.0f;
  return z;
}

// (t * 255).astype(np.uint8) for 0 <= t * 255 < 256: truncation
RPT_HEAT_HD uint8_t chan(float t) {
  const float c = t * 255.0f;
  return (uint8_t)(int32_t)c;
}

// z in [0, 255] -> blue .. cyan .. green .. yellow .. red
RPT_HEAT_HD void rgb(float z, uint8_t* out) {
  const float nz = fdiv(z, 255.0f);
  if (nz < 0.25f) {
    const float t = nz * 4.0f;
    out[0] = 0;
    out[1] = chan(t);
    out[2] = 255;
  } else if (nz < 0.5f) {
    const float t = (nz - 0.25f) * 4.0f;
    out[0] = 0;
    out[1] = 255;
    out[2] = chan(1.0f - t);
  } else if (nz < 0.75f) {
    const float t = (nz - 0.5f) * 4.0f;
    out[0] = chan(t);
    out[1] = 255;
    out[2] = 0;
  } else {  // (a NaN fails every comparison of the script and keeps its zeros; not an input here)
    const float t = (nz - 0.75f) * 4.0f;
    out[0] = 255;
    out[1] = chan(1.0f - t);
    out[2] = 0;
  }
}

}  // namespace heat

// "%.4f" of a float32: v = +-m * 2^ex (m < 2^24; ex = exponent - 150, subnormals -149), so
//   v * 10^4 = m * 625 * 2^(ex + 4)             p = m * 625 < 2^34, s = ex + 4
//   q = p << s            (s >= 0; |v| < 2^40 keeps q < 2^54)
//   q = rne(p >> -s)      (s < 0: half to even on the bits shifted out; 0 once -s >= 36)
// and the text is sign, q / 10^4, '.', q % 10^4 on four digits.  The sign is the sign BIT, so -0.0
// and negatives that round to zero print "-0.0000" as printf does.  At most 19 bytes:
// sign + 13 digits + '.' + 4 digits.
namespace fixed4 {

constexpr int kMaxLen = 19;

struct Dec {
  uint32_t top;  // q / 10^10  (< 2^21)
  uint32_t mid;  // q / 10^4 % 10^6
  uint32_t low;  // q % 10^4   (the four decimals)
  uint32_t neg;  // sign bit
};

RPT_HEAT_HD int ndigits(uint32_t v) {
  int d = 1;
  d += v >= 10u;
  d += v >= 100u;
  d += v >= 1000u;
  d += v >= 10000u;
  d += v >= 100000u;
  d += v >= 1000000u;
  d += v >= 10000000u;
  d += v >= 100000000u;
  d += v >= 1000000000u;
  return d;
}

// false: NaN, inf or |v| >= 2^40 (outside the domain)
RPT_HEAT_HD bool decimal(uint32_t bits, Dec* d) {
  const uint32_t e = (bits >> 23) & 0xffu;
  if (e >= 127u + 40u) {
    *d = Dec{0u, 0u, 0u, 0u};
    return false;
  }
  const uint32_t frac = bits & 0x7fffffu;
  const uint64_t m = e ? (frac | 0x800000u) : frac;
  const int s = (int)(e ? e : 1u) - 150 + 4;
  const uint64_t p = m * 625ull;
  uint64_t q;
  if (s >= 0) {
    q = p << s;
  } else if (-s >= 36) {
    q = 0;  // p < 2^34: below half a unit of the fourth decimal
  } else {
    const int sh = -s;
    q = p >> sh;
    const uint64_t rem = p & ((1ull << sh) - 1ull);
    const uint64_t half = 1ull << (sh - 1);
    q += (rem > half) || (rem == half && (q & 1ull));
  }
  const uint64_t ip = q / 10000ull;
  d->low = (uint32_t)(q - ip * 10000ull);
  const uint64_t t = ip / 1000000ull;
  d->mid = (uint32_t)(ip - t * 1000000ull);
  d->top = (uint32_t)t;
  d->neg = bits >> 31;
  return true;
}

RPT_HEAT_HD int length(const Dec& d) {
  return (int)d.neg + (d.top ? ndigits(d.top) + 6 : ndigits(d.mid)) + 5;
}

// the nd low decimal digits of v, most significant first, at p[0..nd)
RPT_HEAT_HD void put_digits(uint8_t* p, uint32_t v, int nd) {
  for (int k = nd - 1; k >= 0; --k) {
    const uint32_t t = v / 10u;
    p[k] = (uint8_t)('0' + (v - t * 10u));
    v = t;
  }
}

RPT_HEAT_HD uint8_t* put(uint8_t* p, const Dec& d) {
  if (d.neg) *p++ = '-';
  if (d.top) {
    const int nt = ndigits(d.top);
    put_digits(p, d.top, nt);
    put_digits(p + nt, d.mid, 6);
    p += nt + 6;
  } else {
    const int nm = ndigits(d.mid);
    put_digits(p, d.mid, nm);
    p += nm;
  }
  *p++ = '.';
  put_digits(p, d.low, 4);
  return p + 4;
}

}  // namespace fixed4
}  // namespace rpt
