// K2/K3: what more than one stage file of land.hip reads; no kernel, no launcher.
//   kBlock, kMaxEdges   block size of the grid-stride kernels; edge values that fit the LDS stage
//   f2ord               float32 -> order-preserving uint32 (bounds kernels, compaction partials)
//   count_le, clip_idx, count_le_arith, Edges, stage_edges
//                       a point's grid cell by exact comparisons with the float64 edges (the grid
//                       kernels and k_land_keep)
// Reads common.h only.

constexpr int kBlock = 256;
constexpr int kMaxEdges = 4096;  // LDS stage; larger grids fall back to global-memory search

__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// number of edges <= v  (np.searchsorted(edges, v, side='right'))
__device__ __forceinline__ int count_le(const double* e, int ne, double v) {
  int lo = 0, hi = ne;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (e[m] <= v)
      lo = m + 1;
    else
      hi = m;
  }
  return lo;
}

__device__ __forceinline__ int clip_idx(int c, int hi) { return c < 0 ? 0 : (c > hi ? hi : c); }

// count_le for the np.arange edges of the land grid (ascending, e[i] ~ e[0] + i*d): start at the
// arithmetic guess and step to the exact count with true edge comparisons, so the result is the
// binary search's for any ascending edges (NaN -> 0, like count_le) in ~2 loads instead of ~7
// dependent ones.
__device__ __forceinline__ int count_le_arith(const double* e, int ne, double v, double inv_d) {
  const double gd = floor((v - e[0]) * inv_d) + 1.0;
  int g = (gd >= 0.0) ? (gd < (double)ne ? (int)gd : ne) : 0;
  if (!(v == v)) return 0;
  while (g < ne && e[g] <= v) ++g;
  while (g > 0 && e[g - 1] > v) --g;
  return g;
}

// Stage both edge arrays in LDS when they fit.
struct Edges {
  const double* xe;
  const double* ye;
  int nxe, nye;
};
__device__ __forceinline__ Edges stage_edges(const double* xe, int nxe, const double* ye, int nye,
                                             double* lds) {
  Edges E{xe, ye, nxe, nye};
  if (nxe + nye <= kMaxEdges) {
    for (int i = threadIdx.x; i < nxe; i += blockDim.x) lds[i] = xe[i];
    for (int i = threadIdx.x; i < nye; i += blockDim.x) lds[nxe + i] = ye[i];
    __syncthreads();
    E.xe = lds;
    E.ye = lds + nxe;
  }
  return E;
}
