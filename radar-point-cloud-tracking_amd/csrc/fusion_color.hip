// Gain-fusion colours on the device (PointCloudWork/5_gain_fusion_ply_builder.py :276-327):
// normalize_intensity's minimum and 99th percentile per SEGMENT of one float32 array, then z and
// the heat-map colour per point.  A segment is one frame (or one gain of a frame): a group of
// frames concatenated on the device goes through one launch of each kernel.
//
// k_seg_p99: one workgroup of 1024 threads per segment.  np.percentile(seg, 99) reads two
// adjacent order statistics, sorted[lo] and sorted[hi] (heat::rank99); nothing is sorted.  The
// key of sorted[lo] is found by a radix select on heat::key (the order-preserving uint32 image of
// the float bits): four passes over the segment, most significant byte first, each counting the
// candidates (keys that share the bytes chosen so far) by their next byte in a 256-bin LDS
// histogram; wave 0 then scans the histogram and picks the bin that holds the rank.  The passes
// also give count(key < sorted[lo]) and count(key == sorted[lo]), so sorted[hi] is sorted[lo]
// when that many ties reach past index lo, else the smallest key above it (a fifth pass, run only
// then).  The minimum is reduced in the first pass.  The segment stays in L2 between passes; one
// workgroup per segment keeps the kernel free of global atomics and of inter-block ordering.
//
// k_heat: one thread per point: its segment by binary search in the offsets, heat::normalize and
// heat::rgb (heat.h, shared with the host).
#include "common.h"
#include "heat.h"

namespace rpt {
namespace {
constexpr int kSelBlock = 1024;
constexpr int kHeatBlock = 256;

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}

__global__ void __launch_bounds__(kSelBlock)
k_seg_p99(const float* __restrict__ v, int64_t n, const int64_t* __restrict__ seg_off,
          float* __restrict__ seg_min, float* __restrict__ seg_p99) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh_digit, sh_below, sh_cnt, sh_min, sh_next;
  const int tid = (int)threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t a = seg_off[s], b = seg_off[s + 1];
  // empty segment, or offsets that are not this array's: nothing of v is read
  if (a < 0 || b <= a || b > n || b - a > 0x7fffffffll) {
    if (tid == 0) {
      seg_min[s] = 0.0f;
      seg_p99[s] = 0.0f;
    }
    return;
  }
  const float* __restrict__ p = v + a;
  const uint32_t m = (uint32_t)(b - a);
  int64_t lo, hi;
  float t;
  heat::rank99((int64_t)m, &lo, &hi, &t);
  uint32_t r = (uint32_t)lo;  // rank of sorted[lo] among the candidates
  uint32_t prefix = 0, below = 0, cnt_eq = 0;
  uint32_t local_min = 0xffffffffu;
  if (tid == 0) {
    sh_min = 0xffffffffu;
    sh_next = 0xffffffffu;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass ? (0xffffffffu << (shift + 8)) : 0u;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < m; i += kSelBlock) {
      const uint32_t k = heat::key(p[i]);
      if (pass == 0) local_min = min(local_min, k);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: four bins a lane, inclusive scan, the lane whose range holds r
      const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2],
                     h3 = hist[4 * tid + 3];
      const uint32_t sum = h0 + h1 + h2 + h3;
      uint32_t inc = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, off);
        if (tid >= off) inc += up;
      }
      uint32_t e = inc - sum;
      if (r >= e && r < inc) {
        int d = 0;
        uint32_t c = h0;
        if (r >= e + h0) {
          e += h0;
          d = 1;
          c = h1;
          if (r >= e + h1) {
            e += h1;
            d = 2;
            c = h2;
            if (r >= e + h2) {
              e += h2;
              d = 3;
              c = h3;
            }
          }
        }
        sh_digit = (uint32_t)(4 * tid + d);
        sh_below = e;
        sh_cnt = c;
      }
    }
    __syncthreads();
    prefix |= sh_digit << shift;
    r -= sh_below;
    below += sh_below;
    cnt_eq = sh_cnt;
    // (sh_* are rewritten only behind the next pass's two barriers)
  }
  const uint32_t key_lo = prefix;
  // sorted[lo + 1] is another copy of sorted[lo] when the ties reach past index lo
  const bool need_next = hi > lo && (uint64_t)below + cnt_eq <= (uint64_t)lo + 1u;
  uint32_t local_next = 0xffffffffu;
  if (need_next) {
    for (uint32_t i = (uint32_t)tid; i < m; i += kSelBlock) {
      const uint32_t k = heat::key(p[i]);
      if (k > key_lo) local_next = min(local_next, k);
    }
  }
  local_min = wave_min_u32(local_min);
  local_next = wave_min_u32(local_next);
  if ((tid & 63) == 0) {
    atomicMin(&sh_min, local_min);
    if (need_next) atomicMin(&sh_next, local_next);
  }
  __syncthreads();
  if (tid == 0) {
    const float fa = heat::unkey(key_lo);
    const float fb = need_next ? heat::unkey(sh_next) : fa;
    seg_min[s] = heat::unkey(sh_min);
    seg_p99[s] = heat::lerp99(fa, fb, t);
  }
}

__global__ void __launch_bounds__(kHeatBlock)
k_heat(const float* __restrict__ v, int64_t n, const int64_t* __restrict__ seg_off, int64_t n_seg,
       const float* __restrict__ seg_min, const float* __restrict__ seg_p99, int colors_only,
       float* __restrict__ z, uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * kHeatBlock + threadIdx.x;
  if (i >= n) return;
  float zi;
  if (colors_only) {
    zi = v[i];
  } else {
    // the segment of point i: the last offset <= i (empty segments share an offset and lose)
    int64_t lo = 0, hi = n_seg + 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (seg_off[mid] <= i) lo = mid + 1;
      else hi = mid;
    }
    const int64_t s = lo - 1;
    if (s < 0 || s >= n_seg) return;  // a point outside every segment is left alone
    zi = heat::normalize(v[i], seg_min[s], seg_p99[s]);
    z[i] = zi;
  }
  uint8_t c[3];
  heat::rgb(zi, c);
  rgb[3 * i] = c[0];
  rgb[3 * i + 1] = c[1];
  rgb[3 * i + 2] = c[2];
}
}  // namespace
}  // namespace rpt

extern "C" int32_t rpt_segment_percentile99(const float* v, int64_t n, const int64_t* seg_off,
                                            int64_t n_seg, float* seg_min, float* seg_p99,
                                            void* stream) {
  rpt::clear_error();
  if (n < 0 || n_seg < 0 || (n_seg > 0 && (!seg_off || !seg_min || !seg_p99)) ||
      (n > 0 && n_seg > 0 && !v)) {
    rpt::set_error("rpt_segment_percentile99: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31) || n_seg >= (int64_t(1) << 31)) {
    rpt::set_error("rpt_segment_percentile99: n=%lld, n_seg=%lld exceed the int32 index space",
                   (long long)n, (long long)n_seg);
    return RPT_ENOTSUP;
  }
  if (n_seg == 0) return RPT_OK;
  hipStream_t st = rpt::as_stream(stream);
  hipLaunchKernelGGL(rpt::k_seg_p99, dim3((unsigned)n_seg), dim3(rpt::kSelBlock), 0, st, v, n,
                     seg_off, seg_min, seg_p99);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

extern "C" int32_t rpt_heat_colors(const float* v, int64_t n, const int64_t* seg_off,
                                   int64_t n_seg, const float* seg_min, const float* seg_p99,
                                   int32_t colors_only, float* z, uint8_t* rgb, void* stream) {
  rpt::clear_error();
  const bool bad_seg = !colors_only && (n_seg < 0 || !seg_off || !seg_min || !seg_p99 || !z);
  if (n < 0 || (n > 0 && (!v || !rgb || bad_seg))) {
    rpt::set_error("rpt_heat_colors: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31) || n_seg >= (int64_t(1) << 31)) {
    rpt::set_error("rpt_heat_colors: n=%lld, n_seg=%lld exceed the int32 index space",
                   (long long)n, (long long)n_seg);
    return RPT_ENOTSUP;
  }
  if (n == 0) return RPT_OK;
  hipStream_t st = rpt::as_stream(stream);
  const dim3 grid((unsigned)((n + rpt::kHeatBlock - 1) / rpt::kHeatBlock));
  hipLaunchKernelGGL(rpt::k_heat, grid, dim3(rpt::kHeatBlock), 0, st, v, n, seg_off, n_seg,
                     seg_min, seg_p99, (int)(colors_only != 0), z, rgb);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
