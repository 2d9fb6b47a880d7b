// K3 land filter of the public call, launched by land_filter of land.hip in this order:
//   k_land_keep        reads x, y, the edges and land -> keep[i] = 1 unless i's cell is land
//   (exclusive_scan_total_i32: keep -> pos, pos[n] = the kept count)
//   k_land_scatter     keep, pos -> the kept points in order: xo, yo, vo, go, pfo
//   k_new_offsets      pos, frame_off -> new_off[0 .. n_frames]
// Reads land_shared.inc.

__global__ __launch_bounds__(kBlock) void k_land_keep(const float* __restrict__ x,
                                                     const float* __restrict__ y, int64_t n,
                                                     const double* __restrict__ xe, int nxe,
                                                     const double* __restrict__ ye, int nye,
                                                     const uint8_t* __restrict__ land,
                                                     int32_t* __restrict__ keep) {
  __shared__ double lds[kMaxEdges];
  const Edges E = stage_edges(xe, nxe, ye, nye, lds);
  const int ny = nye - 1;
  const double idx_ = 1.0 / (E.xe[1] - E.xe[0]), idy_ = 1.0 / (E.ye[1] - E.ye[0]);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = clip_idx(count_le_arith(E.xe, nxe, (double)x[i], idx_) - 1, nxe - 2);
    const int iy = clip_idx(count_le_arith(E.ye, nye, (double)y[i], idy_) - 1, nye - 2);
    keep[i] = land[(int64_t)ix * ny + iy] ? 0 : 1;
  }
}

__global__ __launch_bounds__(kBlock) void k_land_scatter(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ v,
    const int32_t* __restrict__ g, const int32_t* __restrict__ pf, int64_t n,
    const int32_t* __restrict__ keep, const int32_t* __restrict__ pos, float* __restrict__ xo,
    float* __restrict__ yo, float* __restrict__ vo, int32_t* __restrict__ go,
    int32_t* __restrict__ pfo) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (!keep[i]) continue;
    const int64_t o = pos[i];
    xo[o] = x[i];
    yo[o] = y[i];
    vo[o] = v[i];
    if (go) go[o] = g[i];
    if (pfo) pfo[o] = pf[i];
  }
}

__global__ void k_new_offsets(const int32_t* __restrict__ pos, const int64_t* __restrict__ off,
                              int n_frames, int64_t* __restrict__ out) {
  for (int f = blockIdx.x * blockDim.x + threadIdx.x; f <= n_frames; f += gridDim.x * blockDim.x)
    out[f] = pos[off[f]];
}
