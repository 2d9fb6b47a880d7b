// "%.6f" text rows on the device: the vertex lines of write_ply
// (radar_pipeline/core/writers.py:45-46, one f-string per point) and the rows np.savetxt writes
// for write_labels_csv (:79-81, fmt "%.6f,%.6f,%.6f,%d").
//
// Both reduce to CPython's "%.6f" % float(np.float32(v)): the exact decimal expansion of the
// binary value, rounded half to even at the sixth decimal.  In integers, for v = +-m * 2^ex
// (m < 2^24; ex = exponent - 150, subnormals -149):
//   v * 10^6 = m * 15625 * 2^(ex + 6)           p = m * 15625 < 2^38, s = ex + 6
//   q = p << s            (s >= 0; |v| < 2^40 keeps q < 2^60)
//   q = rne(p >> -s)      (s < 0: half to even on the bits shifted out; 0 once -s >= 40)
// and the text is sign, q / 10^6, '.', q % 10^6 on six digits.  The sign is the sign BIT, so -0.0
// and negatives that round to zero print "-0.000000" as printf does.  No floating point is used.
//
// Two passes around the library's scan: k_text_len (row lengths, out-of-domain rows counted and
// given length 0) -> exclusive scan -> k_text_write.  One thread per row, 256 rows per block.  A
// block's rows are contiguous in the output, so they are staged in LDS (at most 256 * 81 bytes)
// at the same 16-byte phase as their place in out and then copied by the whole block: 16-byte
// vector stores for the aligned interior, byte stores for the ragged head and tail.
//
// A third layout, RPT_TEXT_XYZ_REPR, goes through the same two kernels with another row type: the
// "repr(x),repr(y),repr(z)\n" rows pandas' to_csv writes for float32 columns
// (processors/cartesian.py:46-53), each value the shortest round-trip decimal of repr32.h (at most
// 19 bytes, 60 a row).  Its domain is every finite value.
//
// A fourth, RPT_TEXT_PLY4, are the "%.4f %.4f %.4f %d %d %d\n" rows np.savetxt writes in
// write_ply_fast (PointCloudWork/5_gain_fusion_ply_builder.py:370-403): the same integer method
// with v * 10^4 = m * 625 * 2^(ex + 4) (fixed4 in heat.h, shared with the host), the same domain.
// A value takes at most sign + 13 digits + '.' + 4 digits = 19 bytes, a row
// 3 * 19 + 3 * 3 + 6 = 72.
#include "common.h"
#include "heat.h"
#include "repr32.h"
#include "text.h"

namespace rpt {
namespace {
constexpr int kBlock = 256;
// 3 * (sign + 13 digits + '.' + 6 digits) + 3 * (separator + up to 3 digits) + separators/newline
constexpr int kRowMax = 81;
constexpr int kRowMax4 = 3 * fixed4::kMaxLen + 3 * 3 + 6;  // RPT_TEXT_PLY4
static_assert(kRowMax4 <= kRowMax && 3 * repr32::kMaxLen + 3 <= kRowMax,
              "the staging buffer is sized by the longest row of any layout");
constexpr int kStage = kBlock * kRowMax + 16;  // + the 16-byte phase of the block's first byte

struct Dec {         // |v| * 10^6 rounded, as three base-10^6 limbs
  uint32_t top;      // q / 10^12   (< 2^21)
  uint32_t mid;      // q / 10^6 % 10^6
  uint32_t low;      // q % 10^6    (the six decimals)
  uint32_t neg;      // sign bit
};

__device__ __forceinline__ int ndigits(uint32_t v) {
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
__device__ __forceinline__ bool decimal6(uint32_t bits, Dec* d) {
  const uint32_t e = (bits >> 23) & 0xffu;
  if (e >= 127u + 40u) {
    *d = Dec{0u, 0u, 0u, 0u};
    return false;
  }
  const uint32_t frac = bits & 0x7fffffu;
  const uint64_t m = e ? (frac | 0x800000u) : frac;
  const int s = (int)(e ? e : 1u) - 150 + 6;
  const uint64_t p = m * 15625ull;
  uint64_t q;
  if (s >= 0) {
    q = p << s;
  } else if (-s >= 40) {
    q = 0;  // p < 2^38: below half a unit of the sixth decimal
  } else {
    const int sh = -s;
    q = p >> sh;
    const uint64_t rem = p & ((1ull << sh) - 1ull);
    const uint64_t half = 1ull << (sh - 1);
    q += (rem > half) || (rem == half && (q & 1ull));
  }
  const uint64_t ip = q / 1000000ull;
  d->low = (uint32_t)(q - ip * 1000000ull);
  const uint64_t t = ip / 1000000ull;
  d->mid = (uint32_t)(ip - t * 1000000ull);
  d->top = (uint32_t)t;
  d->neg = bits >> 31;
  return true;
}

__device__ __forceinline__ int float_len(const Dec& d) {
  return (int)d.neg + (d.top ? ndigits(d.top) + 6 : ndigits(d.mid)) + 7;
}

// the nd low decimal digits of v, most significant first, at p[0..nd)
__device__ __forceinline__ void put_digits(uint8_t* p, uint32_t v, int nd) {
  for (int k = nd - 1; k >= 0; --k) {
    const uint32_t t = v / 10u;
    p[k] = (uint8_t)('0' + (v - t * 10u));
    v = t;
  }
}

__device__ __forceinline__ uint8_t* put_float(uint8_t* p, const Dec& d) {
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
  put_digits(p, d.low, 6);
  return p + 6;
}

__device__ __forceinline__ uint8_t* put_u32(uint8_t* p, uint32_t v) {
  const int nd = ndigits(v);
  put_digits(p, v, nd);
  return p + nd;
}

// One row's operands; len < 0 when a coordinate is outside the domain.
struct Row {
  Dec c[3];
  uint32_t t[3];  // PLY: r, g, b; LABELS: |label| in t[0], its sign in t[1]
  int len;
};

struct ReprRow {
  repr32::Dec c[3];
  int len;
};

struct Row4 {
  fixed4::Dec c[3];
  uint32_t t[3];  // r, g, b
  int len;
};

template <int LAYOUT>
struct RowOf {
  typedef Row type;
};
template <>
struct RowOf<RPT_TEXT_PLY4> {
  typedef Row4 type;
};
template <>
struct RowOf<RPT_TEXT_XYZ_REPR> {
  typedef ReprRow type;
};

template <int LAYOUT>
__device__ __forceinline__ void load_row(const float* __restrict__ x, const float* __restrict__ y,
                                         const float* __restrict__ z, const void* __restrict__,
                                         int64_t i, ReprRow* r) {
  const bool okx = repr32::decimal(__float_as_uint(x[i]), &r->c[0]);
  const bool oky = repr32::decimal(__float_as_uint(y[i]), &r->c[1]);
  const bool okz = repr32::decimal(__float_as_uint(z[i]), &r->c[2]);
  // 2 commas + newline
  r->len = okx && oky && okz
               ? 3 + repr32::length(r->c[0]) + repr32::length(r->c[1]) + repr32::length(r->c[2])
               : -1;
}

template <int LAYOUT>
__device__ __forceinline__ void put_row(uint8_t* p, const ReprRow& r) {
  p = repr32::put(p, r.c[0]);
  *p++ = ',';
  p = repr32::put(p, r.c[1]);
  *p++ = ',';
  p = repr32::put(p, r.c[2]);
  *p = '\n';
}

template <int LAYOUT>
__device__ __forceinline__ void load_row(const float* __restrict__ x, const float* __restrict__ y,
                                         const float* __restrict__ z,
                                         const void* __restrict__ tail, int64_t i, Row4* r) {
  const bool okx = fixed4::decimal(__float_as_uint(x[i]), &r->c[0]);
  const bool oky = fixed4::decimal(__float_as_uint(y[i]), &r->c[1]);
  const bool okz = fixed4::decimal(__float_as_uint(z[i]), &r->c[2]);
  const uint8_t* rgb = static_cast<const uint8_t*>(tail) + 3 * i;
  r->t[0] = rgb[0];
  r->t[1] = rgb[1];
  r->t[2] = rgb[2];
  // 5 spaces + newline
  r->len = okx && oky && okz
               ? ndigits(r->t[0]) + ndigits(r->t[1]) + ndigits(r->t[2]) + 6 +
                     fixed4::length(r->c[0]) + fixed4::length(r->c[1]) + fixed4::length(r->c[2])
               : -1;
}

template <int LAYOUT>
__device__ __forceinline__ void put_row(uint8_t* p, const Row4& r) {
  p = fixed4::put(p, r.c[0]);
  *p++ = ' ';
  p = fixed4::put(p, r.c[1]);
  *p++ = ' ';
  p = fixed4::put(p, r.c[2]);
  *p++ = ' ';
  p = put_u32(p, r.t[0]);
  *p++ = ' ';
  p = put_u32(p, r.t[1]);
  *p++ = ' ';
  p = put_u32(p, r.t[2]);
  *p = '\n';
}

template <int LAYOUT>
__device__ __forceinline__ void load_row(const float* __restrict__ x, const float* __restrict__ y,
                                         const float* __restrict__ z,
                                         const void* __restrict__ tail, int64_t i, Row* r) {
  const bool okx = decimal6(__float_as_uint(x[i]), &r->c[0]);
  const bool oky = decimal6(__float_as_uint(y[i]), &r->c[1]);
  const bool okz = decimal6(__float_as_uint(z[i]), &r->c[2]);
  const bool ok = okx && oky && okz;
  int len;
  if (LAYOUT == RPT_TEXT_PLY) {
    const uint8_t* rgb = static_cast<const uint8_t*>(tail) + 3 * i;
    r->t[0] = rgb[0];
    r->t[1] = rgb[1];
    r->t[2] = rgb[2];
    len = ndigits(r->t[0]) + ndigits(r->t[1]) + ndigits(r->t[2]) + 6;  // 5 spaces + newline
  } else {
    const int32_t lab = static_cast<const int32_t*>(tail)[i];
    r->t[1] = lab < 0;
    r->t[0] = lab < 0 ? 0u - (uint32_t)lab : (uint32_t)lab;
    r->t[2] = 0;
    len = (int)r->t[1] + ndigits(r->t[0]) + 4;  // 3 commas + newline
  }
  r->len = ok ? len + float_len(r->c[0]) + float_len(r->c[1]) + float_len(r->c[2]) : -1;
}

template <int LAYOUT>
__device__ __forceinline__ void put_row(uint8_t* p, const Row& r) {
  constexpr uint8_t sep = LAYOUT == RPT_TEXT_PLY ? ' ' : ',';
  p = put_float(p, r.c[0]);
  *p++ = sep;
  p = put_float(p, r.c[1]);
  *p++ = sep;
  p = put_float(p, r.c[2]);
  *p++ = sep;
  if (LAYOUT == RPT_TEXT_PLY) {
    p = put_u32(p, r.t[0]);
    *p++ = ' ';
    p = put_u32(p, r.t[1]);
    *p++ = ' ';
    p = put_u32(p, r.t[2]);
  } else {
    if (r.t[1]) *p++ = '-';
    p = put_u32(p, r.t[0]);
  }
  *p = '\n';
}

template <int LAYOUT>
__global__ void __launch_bounds__(kBlock)
k_text_len(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
           const void* __restrict__ tail, int64_t n, int32_t* __restrict__ lens,
           unsigned long long* __restrict__ n_bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool bad = false;
  if (i < n) {
    typename RowOf<LAYOUT>::type r;
    load_row<LAYOUT>(x, y, z, tail, i, &r);
    bad = r.len < 0;
    lens[i] = bad ? 0 : r.len;
  }
  const uint64_t m = __ballot(bad);
  if (m && lane_id() == 0) atomicAdd(n_bad, (unsigned long long)__popcll(m));
}

template <int LAYOUT>
__global__ void __launch_bounds__(kBlock)
k_text_write(const float* __restrict__ x, const float* __restrict__ y,
             const float* __restrict__ z, const void* __restrict__ tail, int64_t n,
             const int64_t* __restrict__ off, uint8_t* __restrict__ out, int64_t out_bytes) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStage];
  const int64_t first = (int64_t)blockIdx.x * kBlock;
  const int64_t last = min(first + kBlock, n);  // one past the block's rows
  const int64_t b0 = off[first], b1 = off[last];
  // offsets that are not this input's (or an out too small): the block writes nothing
  if (b0 < 0 || b1 < b0 || b1 > out_bytes || b1 - b0 > (int64_t)kBlock * kRowMax) return;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(out) + (uintptr_t)b0;
  const int lo = (int)(a0 & 15u);           // stage[k] is the byte at (a0 - lo) + k
  const int hi = lo + (int)(b1 - b0);
  const int64_t i = first + threadIdx.x;
  if (i < last) {
    typename RowOf<LAYOUT>::type r;
    load_row<LAYOUT>(x, y, z, tail, i, &r);
    const int64_t o = off[i], o1 = off[i + 1];
    // a row is staged only where its own length says it ends, inside the block's range
    if (r.len > 0 && o >= b0 && o1 - o == r.len && o1 <= b1) {
      put_row<LAYOUT>(stage + lo + (int)(o - b0), r);
    } else if (o >= b0 && o1 >= o && o1 <= b1) {
      // skipped row with a consistent slot: defined bytes instead of stale LDS
      for (int64_t k = o; k < o1; ++k) stage[lo + (int)(k - b0)] = ' ';
    }
  }
  __syncthreads();
  uint8_t* base = reinterpret_cast<uint8_t*>(a0 - (uintptr_t)lo);  // 16-byte aligned
  const int vlo = (lo + 15) & ~15, vhi = hi & ~15;
  const int head_end = min(vlo, hi);
  for (int k = lo + (int)threadIdx.x; k < head_end; k += kBlock) base[k] = stage[k];
  for (int k = vlo + 16 * (int)threadIdx.x; k < vhi; k += 16 * kBlock)
    *reinterpret_cast<uint4*>(base + k) = *reinterpret_cast<const uint4*>(stage + k);
  for (int k = max(vhi, vlo) + (int)threadIdx.x; k < hi; k += kBlock) base[k] = stage[k];
}
}  // namespace

int32_t text_rows_size(int32_t layout, const float* x, const float* y, const float* z,
                       const void* tail, int64_t n, int64_t* row_offsets, int64_t* total_host,
                       int64_t* n_bad_host, hipStream_t st) {
  *total_host = 0;
  *n_bad_host = 0;
  if (n == 0) {
    RPT_HIP(hipMemsetAsync(row_offsets, 0, sizeof(int64_t), st));
    return wait_stream(st);
  }
  Scratch& sc = scratch(st);
  Budget bud;
  bud.add<int32_t>(n);
  RPT_TRY(sc.reserve(bud.bytes, st));
  int32_t* lens = sc.carve_n<int32_t>(n);
  unsigned long long* n_bad = nullptr;
  RPT_TRY(zero_n(st, 1, &n_bad));
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (layout == RPT_TEXT_PLY)
    hipLaunchKernelGGL(k_text_len<RPT_TEXT_PLY>, grid, dim3(kBlock), 0, st, x, y, z, tail, n,
                       lens, n_bad);
  else if (layout == RPT_TEXT_LABELS)
    hipLaunchKernelGGL(k_text_len<RPT_TEXT_LABELS>, grid, dim3(kBlock), 0, st, x, y, z, tail, n,
                       lens, n_bad);
  else if (layout == RPT_TEXT_PLY4)
    hipLaunchKernelGGL(k_text_len<RPT_TEXT_PLY4>, grid, dim3(kBlock), 0, st, x, y, z, tail, n,
                       lens, n_bad);
  else
    hipLaunchKernelGGL(k_text_len<RPT_TEXT_XYZ_REPR>, grid, dim3(kBlock), 0, st, x, y, z, tail,
                       n, lens, n_bad);
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i32_to_i64(lens, row_offsets, n, st));
  int64_t tot = 0;
  unsigned long long bad = 0;
  RPT_HIP(hipMemcpyAsync(&tot, row_offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RPT_HIP(hipMemcpyAsync(&bad, n_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  *total_host = tot;
  *n_bad_host = (int64_t)bad;
  return RPT_OK;
}

int32_t text_rows_write(int32_t layout, const float* x, const float* y, const float* z,
                        const void* tail, int64_t n, const int64_t* row_offsets, uint8_t* out,
                        int64_t out_bytes, hipStream_t st) {
  if (n == 0) return RPT_OK;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (layout == RPT_TEXT_PLY)
    hipLaunchKernelGGL(k_text_write<RPT_TEXT_PLY>, grid, dim3(kBlock), 0, st, x, y, z, tail, n,
                       row_offsets, out, out_bytes);
  else if (layout == RPT_TEXT_LABELS)
    hipLaunchKernelGGL(k_text_write<RPT_TEXT_LABELS>, grid, dim3(kBlock), 0, st, x, y, z, tail,
                       n, row_offsets, out, out_bytes);
  else if (layout == RPT_TEXT_PLY4)
    hipLaunchKernelGGL(k_text_write<RPT_TEXT_PLY4>, grid, dim3(kBlock), 0, st, x, y, z, tail,
                       n, row_offsets, out, out_bytes);
  else
    hipLaunchKernelGGL(k_text_write<RPT_TEXT_XYZ_REPR>, grid, dim3(kBlock), 0, st, x, y, z, tail,
                       n, row_offsets, out, out_bytes);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

}  // namespace rpt
