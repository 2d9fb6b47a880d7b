// xy bounds of a point set, launched by bounds_xy of land.hip in this order:
//   k_bounds_xy        reads x, y -> part[4 * block]: min x, max x, min y, max y as f2ord words
//   k_bounds_xy_final  part -> out[0..3], read back and decoded by the host
// Reads land_shared.inc (kBlock, f2ord).

__global__ __launch_bounds__(kBlock) void k_bounds_xy(const float* __restrict__ x,
                                                     const float* __restrict__ y, int64_t n,
                                                     uint32_t* __restrict__ out) {
  uint32_t mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u;
  // kBU points per thread per round, loaded together from clamped indices (a repeated valid
  // point leaves minima and maxima unchanged)
  constexpr int kBU = 4;
  for (int64_t b0 = (int64_t)blockIdx.x * blockDim.x * kBU; b0 < n;
       b0 += (int64_t)gridDim.x * blockDim.x * kBU) {
    float xs[kBU], ys[kBU];
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      const int64_t i = min(b0 + (int64_t)u * blockDim.x + threadIdx.x, n - 1);
      xs[u] = x[i];
      ys[u] = y[i];
    }
#pragma unroll
    for (int u = 0; u < kBU; ++u) {
      const uint32_t a = f2ord(xs[u]), b = f2ord(ys[u]);
      mnx = min(mnx, a);
      mxx = max(mxx, a);
      mny = min(mny, b);
      mxy = max(mxy, b);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mnx = min(mnx, (uint32_t)__shfl_xor((int)mnx, off));
    mxx = max(mxx, (uint32_t)__shfl_xor((int)mxx, off));
    mny = min(mny, (uint32_t)__shfl_xor((int)mny, off));
    mxy = max(mxy, (uint32_t)__shfl_xor((int)mxy, off));
  }
  __shared__ uint32_t sm[kBlock / 64][4];
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x / 64][0] = mnx;
    sm[threadIdx.x / 64][1] = mxx;
    sm[threadIdx.x / 64][2] = mny;
    sm[threadIdx.x / 64][3] = mxy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      mnx = min(mnx, sm[w][0]);
      mxx = max(mxx, sm[w][1]);
      mny = min(mny, sm[w][2]);
      mxy = max(mxy, sm[w][3]);
    }
    // per-block partial; k_bounds_xy_final reduces them (no same-address atomics)
    out[4 * blockIdx.x + 0] = mnx;
    out[4 * blockIdx.x + 1] = mxx;
    out[4 * blockIdx.x + 2] = mny;
    out[4 * blockIdx.x + 3] = mxy;
  }
}

__global__ __launch_bounds__(kBlock) void k_bounds_xy_final(const uint32_t* __restrict__ part,
                                                           int nb, uint32_t* __restrict__ out) {
  uint32_t v[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    v[0] = min(v[0], part[4 * b + 0]);
    v[1] = max(v[1], part[4 * b + 1]);
    v[2] = min(v[2], part[4 * b + 2]);
    v[3] = max(v[3], part[4 * b + 3]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v[0] = min(v[0], (uint32_t)__shfl_xor((int)v[0], off));
    v[1] = max(v[1], (uint32_t)__shfl_xor((int)v[1], off));
    v[2] = min(v[2], (uint32_t)__shfl_xor((int)v[2], off));
    v[3] = max(v[3], (uint32_t)__shfl_xor((int)v[3], off));
  }
  __shared__ uint32_t sm[kBlock / 64][4];
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k) sm[threadIdx.x / 64][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      v[0] = min(v[0], sm[w][0]);
      v[1] = max(v[1], sm[w][1]);
      v[2] = min(v[2], sm[w][2]);
      v[3] = max(v[3], sm[w][3]);
    }
    for (int k = 0; k < 4; ++k) out[k] = v[k];
  }
}
