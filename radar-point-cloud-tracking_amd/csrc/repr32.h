// Shortest round-trip decimal text of a float32: what np.float32(v).astype(str) gives and what
// pandas' DataFrame.to_csv writes for a float32 column (processors/cartesian.py:46-53).  One
// routine for the device (csrc/text.hip, layout RPT_TEXT_XYZ_REPR) and the host
// (rpt_float32_repr in csrc/abi.cpp); everything is integer arithmetic.
//
// Digits: v = m2 * 2^e2.  With mv = 4 m2, mp = 4 m2 + 2 and mm = 4 m2 - 1 - mmShift (the half-way
// points to the neighbours; mmShift = 0 just above a power of two, where the lower neighbour is
// half as far), the three are scaled by a power of ten so that the shortest decimal inside
// [mm, mp] can be read off by removing trailing digits while vp / 10 > vm / 10 (Adams, "Ryu: fast
// float-to-string conversion", PLDI 2018).  The scaling is one 32 x 64-bit multiply by a
// truncated power of 5 (or of 1/5) and a shift; the paper shows 59 / 61 table bits are enough for
// every float32.  The interval's end points count as inside when m2 is even (IEEE ties-to-even
// reads them back as v); among the candidates of the shortest length the one nearest v is taken,
// an exact tie going to the even digit.
//
// Text (numpy's rules for repr of a float32):
//   zero                       "0.0" / "-0.0"
//   1e-4 <= |v| < 1e16         positional: integer part (zero-filled up to the point), '.',
//     (on the binary value:    fraction; ".0" when no fraction digit is left; "0." and leading
//      0x38d1b718 <= bits      zeros below 1
//      < 0x5a0e1bca)
//   otherwise                  scientific: d[.ddd]e+XX / e-XX, two exponent digits (|XX| <= 45)
// The longest text is "-9999999000000000.0": 19 bytes.  NaN and inf are outside the domain.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_R32_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RPT_R32_HD inline
#endif

namespace rpt {
namespace repr32 {

constexpr int kMaxLen = 19;
constexpr uint32_t kPosLo = 0x38d1b718u;  // first float32 >= 1e-4 (as a double)
constexpr uint32_t kPosHi = 0x5a0e1bcau;  // first float32 >= 1e16

struct Dec {
  uint32_t digits;  // shortest digit string as an integer (1..9 digits); 0 for +-0
  int32_t exp10;    // |v| = digits * 10^exp10
  int32_t nd;       // number of digits
  uint32_t neg;     // sign bit
  uint32_t sci;     // 1: scientific notation
};

// floor(2^(bits(5^i) - 1 + 59) / 5^i) + 1
RPT_R32_HD uint64_t pow5_inv(int i) {
  constexpr uint64_t t[31] = {
      0x0800000000000001ull, 0x0666666666666667ull, 0x051eb851eb851eb9ull,
      0x04189374bc6a7efaull, 0x068db8bac710cb2aull, 0x053e2d6238da3c22ull,
      0x0431bde82d7b634eull, 0x06b5fca6af2bd216ull, 0x055e63b88c230e78ull,
      0x044b82fa09b5a52dull, 0x06df37f675ef6eaeull, 0x057f5ff85e592558ull,
      0x0465e6604b7a8447ull, 0x0709709a125da071ull, 0x05a126e1a84ae6c1ull,
      0x0480ebe7b9d58567ull, 0x0734aca5f6226f0bull, 0x05c3bd5191b525a3ull,
      0x049c97747490eae9ull, 0x0760f253edb4ab0eull, 0x05e72843249088d8ull,
      0x04b8ed0283a6d3e0ull, 0x078e480405d7b966ull, 0x060b6cd004ac9452ull,
      0x04d5f0a66a23a9dbull, 0x07bcb43d769f762bull, 0x063090312bb2c4efull,
      0x04f3a68dbc8f03f3ull, 0x07ec3daf94180651ull, 0x065697bfa9acd1daull,
      0x051212ffbaf0a7e2ull};
  return t[i];
}

// the top 61 bits of 5^i
RPT_R32_HD uint64_t pow5(int i) {
  constexpr uint64_t t[48] = {
      0x1000000000000000ull, 0x1400000000000000ull, 0x1900000000000000ull,
      0x1f40000000000000ull, 0x1388000000000000ull, 0x186a000000000000ull,
      0x1e84800000000000ull, 0x1312d00000000000ull, 0x17d7840000000000ull,
      0x1dcd650000000000ull, 0x12a05f2000000000ull, 0x174876e800000000ull,
      0x1d1a94a200000000ull, 0x12309ce540000000ull, 0x16bcc41e90000000ull,
      0x1c6bf52634000000ull, 0x11c37937e0800000ull, 0x16345785d8a00000ull,
      0x1bc16d674ec80000ull, 0x1158e460913d0000ull, 0x15af1d78b58c4000ull,
      0x1b1ae4d6e2ef5000ull, 0x10f0cf064dd59200ull, 0x152d02c7e14af680ull,
      0x1a784379d99db420ull, 0x108b2a2c28029094ull, 0x14adf4b7320334b9ull,
      0x19d971e4fe8401e7ull, 0x1027e72f1f128130ull, 0x1431e0fae6d7217cull,
      0x193e5939a08ce9dbull, 0x1f8def8808b02452ull, 0x13b8b5b5056e16b3ull,
      0x18a6e32246c99c60ull, 0x1ed09bead87c0378ull, 0x13426172c74d822bull,
      0x1812f9cf7920e2b6ull, 0x1e17b84357691b64ull, 0x12ced32a16a1b11eull,
      0x178287f49c4a1d66ull, 0x1d6329f1c35ca4bfull, 0x125dfa371a19e6f7ull,
      0x16f578c4e0a060b5ull, 0x1cb2d6f618c878e3ull, 0x11efc659cf7d4b8dull,
      0x166bb7f0435c9e71ull, 0x1c06a5ec5433c60dull, 0x118427b3b4a05bc8ull};
  return t[i];
}

constexpr int kInvBits = 59;
constexpr int kPowBits = 61;

RPT_R32_HD int pow5_bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }  // e <= 3528
RPT_R32_HD int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }       // e <= 1650
RPT_R32_HD int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }      // e <= 2620

// (m * f) >> s for 32 < s < 96; the result fits 32 bits for every operand used below
RPT_R32_HD uint32_t mul_shift(uint32_t m, uint64_t f, int s) {
  const uint64_t lo = (uint64_t)m * (uint32_t)f;
  const uint64_t hi = (uint64_t)m * (uint32_t)(f >> 32);
  return (uint32_t)(((lo >> 32) + hi) >> (s - 32));
}

RPT_R32_HD bool multiple_of_pow5(uint32_t v, int p) {
  int c = 0;
  for (;;) {
    const uint32_t q = v / 5u;
    if (v - 5u * q != 0u) break;
    v = q;
    ++c;
  }
  return c >= p;
}

RPT_R32_HD int count_digits(uint32_t v) {
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

// false: NaN or inf
RPT_R32_HD bool decimal(uint32_t bits, Dec* d) {
  const uint32_t be = (bits >> 23) & 0xffu;
  const uint32_t frac = bits & 0x7fffffu;
  const uint32_t mag = bits & 0x7fffffffu;
  d->neg = bits >> 31;
  d->sci = mag != 0u && (mag < kPosLo || mag >= kPosHi);
  d->digits = 0;
  d->exp10 = 0;
  d->nd = 1;
  if (be == 0xffu) return false;
  if (mag == 0u) return true;

  const uint32_t m2 = be ? (frac | 0x800000u) : frac;
  const int e2 = (int)(be ? be : 1u) - 127 - 23 - 2;
  const bool accept = (m2 & 1u) == 0u;
  const uint32_t mm_shift = frac != 0u || be <= 1u;
  const uint32_t mv = 4u * m2, mp = 4u * m2 + 2u, mm = 4u * m2 - 1u - mm_shift;

  uint32_t vr, vp, vm;
  int e10;
  bool vm_tz = false, vr_tz = false;
  uint32_t last = 0;  // the digit removed last
  if (e2 >= 0) {
    const int q = log10_pow2(e2);
    e10 = q;
    const int k = kInvBits + pow5_bits(q) - 1;
    const int i = -e2 + q + k;
    vr = mul_shift(mv, pow5_inv(q), i);
    vp = mul_shift(mp, pow5_inv(q), i);
    vm = mul_shift(mm, pow5_inv(q), i);
    if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {
      // no digit will be removed in the loop below: the rounding digit comes from one scale down
      const int l = kInvBits + pow5_bits(q - 1) - 1;
      last = mul_shift(mv, pow5_inv(q - 1), -e2 + q - 1 + l) % 10u;
    }
    if (q <= 9) {  // only then can mv, mp or mm be a multiple of 5^q
      if (mv % 5u == 0u) vr_tz = multiple_of_pow5(mv, q);
      else if (accept) vm_tz = multiple_of_pow5(mm, q);
      else vp -= multiple_of_pow5(mp, q);
    }
  } else {
    const int q = log10_pow5(-e2);
    e10 = q + e2;
    const int i = -e2 - q;
    const int k = pow5_bits(i) - kPowBits;
    int j = q - k;
    vr = mul_shift(mv, pow5(i), j);
    vp = mul_shift(mp, pow5(i), j);
    vm = mul_shift(mm, pow5(i), j);
    if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {
      j = q - 1 - (pow5_bits(i + 1) - kPowBits);
      last = mul_shift(mv, pow5(i + 1), j) % 10u;
    }
    if (q <= 1) {
      vr_tz = true;  // mv = 4 m2 has at least two trailing zero bits
      if (accept) vm_tz = mm_shift == 1u;
      else --vp;
    } else if (q < 31) {
      vr_tz = (mv & ((1u << (q - 1)) - 1u)) == 0u;
    }
  }

  int removed = 0;
  uint32_t out;
  if (vm_tz || vr_tz) {  // rare: exact end points or an exact half
    while (vp / 10u > vm / 10u) {
      vm_tz &= vm % 10u == 0u;
      vr_tz &= last == 0u;
      last = vr % 10u;
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      ++removed;
    }
    if (vm_tz) {
      while (vm % 10u == 0u) {
        vr_tz &= last == 0u;
        last = vr % 10u;
        vr /= 10u;
        vp /= 10u;
        vm /= 10u;
        ++removed;
      }
    }
    if (vr_tz && last == 5u && vr % 2u == 0u) last = 4u;  // exact half: to the even digit
    out = vr + (((vr == vm) && (!accept || !vm_tz)) || last >= 5u);
  } else {
    while (vp / 10u > vm / 10u) {
      last = vr % 10u;
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      ++removed;
    }
    out = vr + (vr == vm || last >= 5u);
  }
  d->digits = out;
  d->exp10 = e10 + removed;
  d->nd = count_digits(out);
  return true;
}

// bytes of the text of a value decimal() accepted
RPT_R32_HD int length(const Dec& d) {
  const int s = (int)d.neg;
  if (d.digits == 0u) return s + 3;
  if (d.sci) return s + d.nd + (d.nd > 1) + 4;
  if (d.exp10 >= 0) return s + d.nd + d.exp10 + 2;
  if (d.nd + d.exp10 > 0) return s + d.nd + 1;
  return s + 2 - d.exp10;
}

// the nd low decimal digits of v, most significant first, at p[0..nd)
RPT_R32_HD void put_digits(uint8_t* p, uint32_t v, int nd) {
  for (int k = nd - 1; k >= 0; --k) {
    const uint32_t t = v / 10u;
    p[k] = (uint8_t)('0' + (v - t * 10u));
    v = t;
  }
}

// writes length(d) bytes at p, returns the byte after them
RPT_R32_HD uint8_t* put(uint8_t* p, const Dec& d) {
  if (d.neg) *p++ = '-';
  if (d.digits == 0u) {
    *p++ = '0';
    *p++ = '.';
    *p++ = '0';
    return p;
  }
  if (d.sci) {
    if (d.nd > 1) {
      put_digits(p + 1, d.digits, d.nd);  // digits one place to the right,
      p[0] = p[1];                        // then the first in front of the point
      p[1] = '.';
      p += d.nd + 1;
    } else {
      *p++ = (uint8_t)('0' + d.digits);
    }
    int e = d.exp10 + d.nd - 1;
    *p++ = 'e';
    *p++ = e < 0 ? '-' : '+';
    if (e < 0) e = -e;
    *p++ = (uint8_t)('0' + e / 10);
    *p++ = (uint8_t)('0' + e % 10);
    return p;
  }
  if (d.exp10 >= 0) {
    put_digits(p, d.digits, d.nd);
    p += d.nd;
    for (int k = 0; k < d.exp10; ++k) *p++ = '0';
    *p++ = '.';
    *p++ = '0';
    return p;
  }
  const int ip = d.nd + d.exp10;  // digits in front of the point
  if (ip > 0) {
    put_digits(p + 1, d.digits, d.nd);
    for (int k = 0; k < ip; ++k) p[k] = p[k + 1];
    p[ip] = '.';
    return p + d.nd + 1;
  }
  *p++ = '0';
  *p++ = '.';
  for (int k = 0; k < -ip; ++k) *p++ = '0';
  put_digits(p, d.digits, d.nd);
  return p + d.nd;
}

}  // namespace repr32
}  // namespace rpt
