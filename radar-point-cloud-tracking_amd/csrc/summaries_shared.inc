// K9: what more than one stage file of summaries.hip reads.  No launcher of its own except
// k_fill_i64 (fill_noise of summaries_impl: frame_first_noise = -1 and, on the frame-sort path,
// the two counters [overflow flag, long-run count] cleared in the same launch).
//   kBlock              block size of every grid-stride kernel and of the run kernels
//   to_float / load4    intensity reads, float32 or u8 (the kernels' VT), converted on load
//   lower_bound_i32     wave-wide 64-ary search in the per-point frame slots
//   FramesPf, FramesOff where the frames' points lie (the kernels' FR): k_heads, the run kernels'
//                       metadata and both frame sorts read them
//   wave_incl_scan      wave-inclusive scan of one value per lane (both frame sorts)
// Reads common.h and frame_index.h (frame_of_point).

constexpr int kBlock = 256;

// Intensities are float32 or -- the stack driver's narrow path, u8 echo samples -- uint8_t (the
// kernels' VT): every read converts on load.
__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(uint8_t v) { return (float)v; }
// four consecutive intensities at p + 4 q (p aligned to four elements)
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int q) {
  return reinterpret_cast<const float4*>(p)[q];
}
__device__ __forceinline__ float4 load4(const uint8_t* __restrict__ p, int q) {
  const uint32_t w = reinterpret_cast<const uint32_t*>(p)[q];
  return make_float4((float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu),
                     (float)(w >> 24));
}

// first index with a[i] >= key in the non-decreasing a[0, n), by the WHOLE wave (uniform
// arguments, every lane active; the result is uniform): a 64-ary search, 64 probes per round, ~5
// dependent rounds over a 50 M-point stack where a thread's binary search took 26 -- the frame
// sort blocks began with two such searches each
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t n,
                                                   int32_t key) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = n;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t idx = lo + (int64_t)lane * step;
    const bool below = idx < hi && a[idx < hi ? idx : lo] < key;  // a prefix of the lanes
    const int c = __popcll(__ballot(below));
    if (c == 0) {
      hi = lo;
    } else {
      const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
      hi = min(hi, lo + (int64_t)c * step);
      lo = nlo;
    }
  }
  return lo;
}

// Where the frames' points lie in the frame-major point order, two forms (the kernels' FR):
// per-point frame slots (the public call and the shard driver) or the frame offsets
// off[0 .. F] of the same points (the stack driver's narrow path, which keeps no slots).
// begin(n, f): first point of frame slot >= f, by the whole wave (uniform f, f <= F);
// frame(i): frame slot of point i.
struct FramesPf {
  const int32_t* __restrict__ pf;
  __device__ __forceinline__ int begin(int64_t n, int f) const {
    return (int)lower_bound_i32(pf, n, f);
  }
  __device__ __forceinline__ int32_t frame(int64_t i) const { return pf[i]; }
};
struct FramesOff {
  const int64_t* __restrict__ off;
  int32_t F;
  __device__ __forceinline__ int begin(int64_t, int f) const { return (int)off[f]; }
  __device__ __forceinline__ int32_t frame(int64_t i) const { return frame_of_point(off, F, i); }
};

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(x, off);
    if (lane >= off) x += o;
  }
  return x;
}

// p[0, n) = v; zero2 (nullable): two counters of the next kernel cleared (no memset launch)
__global__ void k_fill_i64(int64_t* p, int64_t n, int64_t v, int32_t* zero2 = nullptr) {
  if (zero2 && blockIdx.x == 0 && threadIdx.x < 2) zero2[threadIdx.x] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}
