// K2 occupancy grid and land mask.  land_grid_cells_t of land.hip zeroes cnt / tot (k_zero_land,
// defined there) and launches ONE of the three grid kernels; each reads x, y, val and the edges
// xe / ye and leaves cnt[cell] (int32 counts), tot[cell] (float64 intensity sums) and, when
// cell_out is given, every point's cell:
//   k_land_grid_lds_u8<CT, VT>  u8-valued points, grid + edges within 150 KiB of LDS: count and
//                               sum packed in one 64-bit LDS atomic per point
//   k_land_grid_lds<CT, VT>     up to kLdsGridCells cells: LDS-privatised counts and sums
//   k_land_grid<CT, VT>         any grid: global atomics, edges in LDS when they fit
// land_mask_dev launches k_land_mask: cnt, tot -> land[cell] (0 / 1) and *n_land.
// Reads land_shared.inc.

// LDS-privatised form: int32 counts + f64 sums of the whole grid per block (fits when
// cells * 12 B + edges <= ~150 KiB), flushed with one atomic per non-empty cell.  One 1024-thread
// block per CU: the per-block cost (zeroing and flushing ~10k cells) is paid 256 times, not once
// per 256-thread block of a larger grid, and 16 waves per CU hide the LDS atomics' latency.
constexpr int kLdsGridCells = 10240;
constexpr int kGridBlock = 1024;
// CT (all three grid kernels): the element type of cell_out, int32_t or -- the stack driver's
// narrow path, grids of at most 65,536 cells -- uint16_t; VT: the element type of val, float
// or -- the narrow path's u8 samples -- uint8_t
template <class CT, class VT>
__global__ __launch_bounds__(kGridBlock) void k_land_grid_lds(const float* __restrict__ x,
                                                         const float* __restrict__ y,
                                                         const VT* __restrict__ val, int64_t n,
                                                         const double* __restrict__ xe, int nxe,
                                                         const double* __restrict__ ye, int nye,
                                                         int32_t* __restrict__ cnt,
                                                         double* __restrict__ tot,
                                                         CT* __restrict__ cell_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lds_e = reinterpret_cast<double*>(smem);                    // nxe + nye edges
  const int ne = nxe + nye;
  const int ne_al = (ne + 1) & ~1;
  double* lds_t = lds_e + ne_al;                                       // cells f64 sums
  const int ny = nye - 1;
  const int cells = (nxe - 1) * ny;
  int32_t* lds_c = reinterpret_cast<int32_t*>(lds_t + cells);          // cells counts
  for (int i = threadIdx.x; i < nxe; i += blockDim.x) lds_e[i] = xe[i];
  for (int i = threadIdx.x; i < nye; i += blockDim.x) lds_e[nxe + i] = ye[i];
  for (int c = threadIdx.x; c < cells; c += blockDim.x) {
    lds_t[c] = 0.0;
    lds_c[c] = 0;
  }
  __syncthreads();
  const double* ex = lds_e;
  const double* ey = lds_e + nxe;
  const double idx_ = 1.0 / (ex[1] - ex[0]), idy_ = 1.0 / (ey[1] - ey[0]);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = clip_idx(count_le_arith(ex, nxe, (double)x[i], idx_) - 1, nxe - 2);
    const int iy = clip_idx(count_le_arith(ey, nye, (double)y[i], idy_) - 1, nye - 2);
    const int c = ix * ny + iy;
    if (cell_out) cell_out[i] = (CT)c;
    atomicAdd(lds_c + c, 1);
    atomicAdd(lds_t + c, (double)val[i]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += blockDim.x) {
    const int k = lds_c[c];
    if (k) {
      atomicAdd(cnt + c, k);
      atomicAdd(tot + c, lds_t[c]);
    }
  }
}

// Same, for intensities that are integers in [0, 255] (u8 echo samples): one packed u64 LDS
// atomic per point, count << 40 | sum (a block's per-cell count < 2^24 and sum < 2^40, checked by
// the caller), instead of an int32 and a float64 atomic.  Integer sums below 2^53 are exact in any
// order, so the float64 grid equals the unpacked kernel's.
constexpr int kPackShift = 40;
template <class CT, class VT>
__global__ __launch_bounds__(kGridBlock) void k_land_grid_lds_u8(
    const float* __restrict__ x, const float* __restrict__ y, const VT* __restrict__ val,
    int64_t n, const double* __restrict__ xe, int nxe, const double* __restrict__ ye, int nye,
    int32_t* __restrict__ cnt, double* __restrict__ tot, CT* __restrict__ cell_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lds_e = reinterpret_cast<double*>(smem);  // nxe + nye edges
  const int ne = nxe + nye;
  const int ne_al = (ne + 1) & ~1;
  unsigned long long* lds_p = reinterpret_cast<unsigned long long*>(lds_e + ne_al);
  const int ny = nye - 1;
  const int cells = (nxe - 1) * ny;
  for (int i = threadIdx.x; i < nxe; i += blockDim.x) lds_e[i] = xe[i];
  for (int i = threadIdx.x; i < nye; i += blockDim.x) lds_e[nxe + i] = ye[i];
  for (int c = threadIdx.x; c < cells; c += blockDim.x) lds_p[c] = 0ull;
  __syncthreads();
  const double* ex = lds_e;
  const double* ey = lds_e + nxe;
  const double idx_ = 1.0 / (ex[1] - ex[0]), idy_ = 1.0 / (ey[1] - ey[0]);
  // one 1024-thread block per CU: kU points per thread per round, loads issued together (16
  // waves alone keep too few bytes in flight)
  constexpr int kU = 8;
  const int64_t chunk = (int64_t)kGridBlock * kU;
  for (int64_t b0 = (int64_t)blockIdx.x * chunk; b0 < n; b0 += (int64_t)gridDim.x * chunk) {
    float px[kU], py[kU];
    VT pv[kU];
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      const int64_t i = min(b0 + (int64_t)k * kGridBlock + threadIdx.x, n - 1);  // branch-free
      px[k] = x[i];
      py[k] = y[i];
      pv[k] = val[i];
    }
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      const int64_t i = b0 + (int64_t)k * kGridBlock + threadIdx.x;
      if (i >= n) break;
      const int ix = clip_idx(count_le_arith(ex, nxe, (double)px[k], idx_) - 1, nxe - 2);
      const int iy = clip_idx(count_le_arith(ey, nye, (double)py[k], idy_) - 1, nye - 2);
      const int c = ix * ny + iy;
      if (cell_out) cell_out[i] = (CT)c;
      atomicAdd(lds_p + c, (1ull << kPackShift) | (unsigned long long)(uint32_t)pv[k]);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += blockDim.x) {
    const unsigned long long v = lds_p[c];
    if (v) {
      atomicAdd(cnt + c, (int32_t)(v >> kPackShift));
      atomicAdd(tot + c, (double)(v & ((1ull << kPackShift) - 1ull)));
    }
  }
}

template <class CT, class VT>
__global__ __launch_bounds__(kBlock) void k_land_grid(const float* __restrict__ x,
                                                     const float* __restrict__ y,
                                                     const VT* __restrict__ val, int64_t n,
                                                     const double* __restrict__ xe, int nxe,
                                                     const double* __restrict__ ye, int nye,
                                                     int32_t* __restrict__ cnt,
                                                     double* __restrict__ tot,
                                                     CT* __restrict__ cell_out) {
  __shared__ double lds[kMaxEdges];
  const Edges E = stage_edges(xe, nxe, ye, nye, lds);
  const int ny = nye - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ix = clip_idx(count_le(E.xe, nxe, (double)x[i]) - 1, nxe - 2);
    const int iy = clip_idx(count_le(E.ye, nye, (double)y[i]) - 1, nye - 2);
    const int64_t c = (int64_t)ix * ny + iy;
    if (cell_out) cell_out[i] = (CT)c;
    atomicAdd(cnt + c, 1);
    atomicAdd(tot + c, (double)val[i]);
  }
}

// identify_land_cells :400-408, all float64
__global__ void k_land_mask(const int32_t* __restrict__ cnt, const double* __restrict__ tot,
                            int64_t cells, double nf, double pthr, double ithr,
                            uint8_t* __restrict__ land, int32_t* __restrict__ n_land) {
  int local = 0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells;
       c += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = cnt[c];
    const double pers = (double)k / nf;
    const double avg = (k > 0) ? tot[c] / (double)k : 0.0;
    const bool is_land = (pers >= pthr) && (avg >= ithr);
    land[c] = is_land ? 1 : 0;
    local += is_land ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(n_land, local);
}
