// Shard driver, the small kernels around the land grid's bounds and counts.  Reads no stage file.
//   rpt_shard_polar      k_init_bounds -> k_xy_bounds_part, only when the K1 write did not leave
//                        the bounds itself: reads the K1 points' x / y (and the count on the
//                        device while the write is speculative), leaves the ordered-u32
//                        {min x, max x, min y, max y} in the handle's bnd
//   rpt_shard_land_grid  k_cnt_to_f64: the own land counts (int32) as float64 in front of the
//                        sums, the buffer the caller all-reduces
//   rpt_shard_halo       k_f64_to_cnt: the reduced counts back to int32 (and the land mask's cell
//                        counter cleared); k_empty_bounds: the own points' ST-DBSCAN bounds when
//                        this rank has no K1 point (the compaction, which writes them, is skipped)

// ordered-u32 min/max of x and y over [0, *n_dev) (n_dev on the device, grid sized for n_max)
__global__ void k_xy_bounds_part(const float* __restrict__ x, const float* __restrict__ y,
                                 int64_t n_max, const int64_t* __restrict__ n_dev,
                                 uint32_t* __restrict__ part) {
  const int64_t n = n_dev ? min(*n_dev, n_max) : n_max;  // speculative: never past n_max
  uint32_t mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t ux = __float_as_uint(x[i]), uy = __float_as_uint(y[i]);
    ux = (ux & 0x80000000u) ? ~ux : (ux | 0x80000000u);
    uy = (uy & 0x80000000u) ? ~uy : (uy | 0x80000000u);
    mnx = min(mnx, ux);
    mxx = max(mxx, ux);
    mny = min(mny, uy);
    mxy = max(mxy, uy);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mnx = min(mnx, (uint32_t)__shfl_xor((int)mnx, off));
    mxx = max(mxx, (uint32_t)__shfl_xor((int)mxx, off));
    mny = min(mny, (uint32_t)__shfl_xor((int)mny, off));
    mxy = max(mxy, (uint32_t)__shfl_xor((int)mxy, off));
  }
  // one set of atomics per block (per-wave atomics on 4 words serialise: ~0.4 ms at 2k blocks)
  __shared__ uint32_t red[4][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = mnx;
    red[1][w] = mxx;
    red[2][w] = mny;
    red[3][w] = mxy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
      mnx = min(mnx, red[0][k]);
      mxx = max(mxx, red[1][k]);
      mny = min(mny, red[2][k]);
      mxy = max(mxy, red[3][k]);
    }
    atomicMin(part + 0, mnx);
    atomicMax(part + 1, mxx);
    atomicMin(part + 2, mny);
    atomicMax(part + 3, mxy);
  }
}

__global__ void k_init_bounds(uint32_t* part) {
  if (threadIdx.x == 0) {
    part[0] = 0xffffffffu;
    part[1] = 0u;
    part[2] = 0xffffffffu;
    part[3] = 0u;
  }
}

// the bounds of no point (the identity of k_bounds_final's reduction)
__global__ void k_empty_bounds(Bounds* __restrict__ out) {
  if (threadIdx.x == 0) {
    Bounds b;
    for (int k = 0; k < 4; ++k) {
      b.mn[k] = 0xffffffffu;
      b.mx[k] = 0u;
    }
    b.nonfinite_xyz = b.nonintegral_t = b.n_finite_t = b.t_descends = 0;
    *out = b;
  }
}

// land grid [counts | sums] in float64 for the all-reduce (integer-valued: exact in any order)
__global__ void k_cnt_to_f64(const int32_t* __restrict__ cnt, int64_t cells,
                             double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (double)cnt[i];
}
__global__ void k_f64_to_cnt(const double* __restrict__ in, int64_t cells,
                             int32_t* __restrict__ cnt, int64_t* __restrict__ zero) {
  // zero: the land mask's cell counter, cleared here instead of by a memset launch
  if (blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells;
       i += (int64_t)gridDim.x * blockDim.x)
    cnt[i] = (int32_t)in[i];
}
