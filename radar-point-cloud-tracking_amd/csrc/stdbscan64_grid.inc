// stdbscan64.hip, the grid build: bounds, cell keys, the sorted points and the cells' starts.
// Reads stdbscan64_shared.inc.  Leaves behind: Bounds64 (read back by the driver), then the
// sorted points (Pts64), sorig (sorted -> original index), skey (sorted -> cell) and
// cell_start[0 .. cells + 1] (cell c's points are [cell_start[c], cell_start[c + 1]); the
// isolated cell is number `cells`).

struct Bounds64 {
  double mn[4], mx[4];    // x, y, z, t over the finite values; +inf / -inf where there is none
  int64_t n_finite_t;
  int32_t nonfinite_xyz;  // any NaN or infinite coordinate
  int32_t pad;
};

__device__ __forceinline__ double time_at(const void* __restrict__ t, bool f64, int64_t i) {
  return f64 ? static_cast<const double*>(t)[i] : (double)static_cast<const float*>(t)[i];
}

__device__ __forceinline__ void bounds_merge(Bounds64& a, const Bounds64& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.mn[k] = fmin(a.mn[k], b.mn[k]);
    a.mx[k] = fmax(a.mx[k], b.mx[k]);
  }
  a.n_finite_t += b.n_finite_t;
  a.nonfinite_xyz |= b.nonfinite_xyz;
}

// every thread of the block calls this; thread 0 stores the block's Bounds64
__device__ __forceinline__ void bounds_block_store(Bounds64 a, Bounds64* __restrict__ out) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Bounds64 b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b.mn[k] = __shfl_xor(a.mn[k], off);
      b.mx[k] = __shfl_xor(a.mx[k], off);
    }
    b.n_finite_t = __shfl_xor(a.n_finite_t, off);
    b.nonfinite_xyz = __shfl_xor(a.nonfinite_xyz, off);
    bounds_merge(a, b);
  }
  __shared__ Bounds64 sb[kBlock / 64];
  if ((threadIdx.x & 63) == 0) sb[threadIdx.x / 64] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    Bounds64 o = sb[0];
    for (int w = 1; w < kBlock / 64; ++w) bounds_merge(o, sb[w]);
    o.pad = 0;
    *out = o;
  }
}

__device__ __forceinline__ Bounds64 bounds_empty() {
  Bounds64 a;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a.mn[k] = INFINITY;
    a.mx[k] = -INFINITY;
  }
  a.n_finite_t = 0;
  a.nonfinite_xyz = 0;
  a.pad = 0;
  return a;
}

// one partial per block (part[gridDim.x])
template <int D>
__global__ __launch_bounds__(kBlock) void k64_bounds(const double* __restrict__ x,
                                                    const double* __restrict__ y,
                                                    const double* __restrict__ z, int64_t stride,
                                                    const void* __restrict__ t, bool tf64,
                                                    int64_t n, Bounds64* __restrict__ part) {
  Bounds64 a = bounds_empty();
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += ts) {
    const double v[4] = {x[i * stride], y[i * stride], D == 3 ? z[i * stride] : 0.0,
                         time_at(t, tf64, i)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (isfinite(v[k])) {
        a.mn[k] = fmin(a.mn[k], v[k]);
        a.mx[k] = fmax(a.mx[k], v[k]);
        if (k == 3) ++a.n_finite_t;
      } else if (k < 3) {
        a.nonfinite_xyz = 1;
      }
    }
  }
  bounds_block_store(a, part + blockIdx.x);
}

// one block: the partials -> out[0]
__global__ __launch_bounds__(kBlock) void k64_bounds_final(const Bounds64* __restrict__ part,
                                                          int nb, Bounds64* __restrict__ out) {
  Bounds64 a = bounds_empty();
  for (int i = threadIdx.x; i < nb; i += kBlock) bounds_merge(a, part[i]);
  bounds_block_store(a, out);
}

// keys[i] = the cell of point i (the isolated cell for a non-finite time), vals[i] = i
template <int D>
__global__ __launch_bounds__(kBlock) void k64_keys(const double* __restrict__ x,
                                                  const double* __restrict__ y,
                                                  const double* __restrict__ z, int64_t stride,
                                                  const void* __restrict__ t, bool tf64, int64_t n,
                                                  Geom64 g, uint32_t* __restrict__ keys,
                                                  uint32_t* __restrict__ vals) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += ts) {
    const double tv = time_at(t, tf64, i);
    int32_t c = g.cells;
    if (isfinite(tv)) {
      const int cx = grid64_index(x[i * stride], g.ox, g.cs, g.nx);
      const int cy = grid64_index(y[i * stride], g.oy, g.cs, g.ny);
      const int cz = D == 3 ? grid64_index(z[i * stride], g.oz, g.cs, g.nz) : 0;
      const int ct = grid64_index(tv, g.ot, g.ct, g.nt);
      c = ((ct * g.nz + cz) * g.ny + cy) * g.nx + cx;  // < cells <= 2^30
    }
    keys[i] = (uint32_t)c;
    vals[i] = (uint32_t)i;
  }
}

// the sorted points from the sorted (cell, original index) pairs
template <int D>
__global__ __launch_bounds__(kBlock) void k64_gather(const double* __restrict__ x,
                                                    const double* __restrict__ y,
                                                    const double* __restrict__ z, int64_t stride,
                                                    const void* __restrict__ t, bool tf64,
                                                    int64_t n, const uint32_t* __restrict__ sk,
                                                    const uint32_t* __restrict__ sv,
                                                    double* __restrict__ sx,
                                                    double* __restrict__ sy,
                                                    double* __restrict__ sz,
                                                    double* __restrict__ stime,
                                                    int32_t* __restrict__ sorig,
                                                    int32_t* __restrict__ skey) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += ts) {
    const int64_t o = sv[s];
    sx[s] = x[o * stride];
    sy[s] = y[o * stride];
    if (D == 3) sz[s] = z[o * stride];
    stime[s] = time_at(t, tf64, o);
    sorig[s] = (int32_t)o;
    skey[s] = (int32_t)sk[s];
  }
}

// cell_start[c] for c in [0, n_cells]: the first sorted point whose cell is >= c (n when none),
// by a binary search per cell.  Every entry is written; an empty cell gets its successor's start.
__global__ __launch_bounds__(kBlock) void k64_cell_start(const int32_t* __restrict__ skey,
                                                        int32_t n, int64_t n_cells,
                                                        int32_t* __restrict__ cell_start) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c <= n_cells; c += ts) {
    int32_t lo = 0, hi = n;  // the answer is in [lo, hi]
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo) / 2;
      if ((int64_t)skey[mid] < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    cell_start[c] = lo;
  }
}
