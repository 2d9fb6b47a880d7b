// Per-label group means (count, x, y, intensity), launched by label_means of summaries.hip after
// radix_front (head kernel k_label_heads):
//   k_label_means   reads sk, seg_start, *n_seg_dev, gx, gy, gi; three waves per label run ->
//                   o_count, o_x, o_y, o_v indexed by label (zeroed beforehand: labels without
//                   points keep count 0)
// The reduction order is pandas' groupby mean (kahan_mean below), not numpy's.
// Reads summaries_shared.inc (kBlock).

// pandas groupby(...).mean() of float32 columns (pandas/_libs/groupby.pyx group_mean, pandas
// 2.x): per group, in row order, a float32 Kahan-compensated sum (y = v - c; t = s + y;
// c = (t - s) - y; c = 0 if NaN; s = t), then s / (float)count.  One wave per run: lanes stage
// chunks in LDS, lane 0 runs the dependent chain.
__device__ __forceinline__ float kahan_mean(const float* __restrict__ g, int b, int e, int lane,
                                            float* __restrict__ sb) {
  constexpr int kPre = 16, kChunk = 64 * kPre;
  float s = 0.f, c = 0.f;
  for (int c0 = b; c0 < e; c0 += kChunk) {
#pragma unroll
    for (int t = 0; t < kPre; ++t) {
      const int idx = c0 + t * 64 + lane;
      sb[t * 64 + lane] = (idx < e) ? g[idx] : 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int m = (e - c0 < kChunk) ? (e - c0) : kChunk;
    if (lane == 0)
      for (int i = 0; i < m; ++i) {
        const float y = sb[i] - c;
        const float t = s + y;
        c = (t - s) - y;
        if (c != c) c = 0.f;
        s = t;
      }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  return s / (float)(e - b);
}

// Three waves per label run: x, y, intensity group means; outputs indexed by label.
__global__ __launch_bounds__(kBlock) void k_label_means(
    const uint32_t* __restrict__ sk, const int64_t* __restrict__ seg_start,
    const int32_t* __restrict__ n_seg_dev, int64_t n, const float* __restrict__ gx,
    const float* __restrict__ gy, const float* __restrict__ gi, int64_t n_labels,
    int64_t* __restrict__ o_count, float* __restrict__ o_x, float* __restrict__ o_y,
    float* __restrict__ o_v) {
  __shared__ float s_buf[kBlock / 64][1024];
  const int64_t n_seg = *n_seg_dev;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t w = w0; w < 3 * n_seg; w += nw) {
    const int su = __builtin_amdgcn_readfirstlane((int)(w / 3));
    const int comp = __builtin_amdgcn_readfirstlane((int)(w - (int64_t)su * 3));
    const int b = __builtin_amdgcn_readfirstlane((int)seg_start[su]);
    const int e = __builtin_amdgcn_readfirstlane(
        (int)((su + 1 < n_seg) ? seg_start[su + 1] : n));
    const int64_t lab = (int64_t)sk[b] - 1;
    const float m = kahan_mean(comp == 0 ? gx : (comp == 1 ? gy : gi), b, e, lane,
                               s_buf[threadIdx.x / 64]);
    if (lane == 0 && lab < n_labels) {
      if (comp == 0) {
        o_x[lab] = m;
        o_count[lab] = e - b;
      } else if (comp == 1) {
        o_y[lab] = m;
      } else {
        o_v[lab] = m;
      }
    }
  }
}
