// K2/K3: land (persistent background) filter.  Replaces build_occupancy_grid, identify_land_cells
// and filter_land_from_frame (PointCloudWork/4_temporal_object_tracker.py:359-436).
//
// Grid semantics are numpy's: edges are the float64 np.arange(min, max + res, res) the host
// builds from the float32 bounds (rpt_bounds_xy); a point's cell is
// clip(searchsorted(edges, v, 'right') - 1, 0, n_edges - 2) — an exact binary search over the
// edge array staged in LDS, so no floating-point re-derivation of the edges can disagree.
// Counts are int32 atomics (order-free); intensity sums are float64 atomics, exact for the
// integer echo values of the radar path (sums < 2^53), like np.add.at's sequential order.
//
// This file is the one translation unit: the host drivers and k_zero_land (defined in namespace
// rpt, beside land_grid_cells_t).  Every other kernel and device helper is in a stage file,
// included (inside namespace rpt { namespace {) in this order; a stage file reads
// land_shared.inc and no other stage file.  Each file's header names the host function that
// launches its kernels, in what order, and what they read and leave behind.
//   land_shared.inc   kBlock, kMaxEdges, f2ord, the edge searches, Edges / stage_edges
//   land_bounds.inc   k_bounds_xy, k_bounds_xy_final (bounds_xy)
//   land_grid.inc     the three k_land_grid* kernels (land_grid_cells_t), k_land_mask
//   land_filter.inc   k_land_keep, k_land_scatter, k_new_offsets (land_filter)
//   land_compact.inc  tile counts, k_land_compact, new offsets, bounds (land_compact_dev)
#include <climits>
#include <cstdlib>
#include <cstring>

#include <algorithm>

#include "common.h"
#include "frame_index.h"
#include "land.h"

#pragma clang fp contract(off)

namespace rpt {
namespace {

#include "land_shared.inc"
#include "land_bounds.inc"
#include "land_grid.inc"
#include "land_filter.inc"
#include "land_compact.inc"

}  // namespace

int32_t bounds_xy(const float* x, const float* y, int64_t n, float* out4, hipStream_t st) {
  if (n <= 0) {
    set_error("zero-size array to reduction operation minimum which has no identity");
    return RPT_EEMPTY;
  }
  const int nb = grid_for(n, kBlock, 1024);
  Scratch& sc = scratch(st);
  Budget bud;
  bud.add<uint32_t>(4);
  bud.add<uint32_t>(4 * (int64_t)nb);
  RPT_TRY(sc.reserve(bud.bytes, st));
  uint32_t* d = sc.carve_n<uint32_t>(4);
  uint32_t* part = sc.carve_n<uint32_t>(4 * (int64_t)nb);
  hipLaunchKernelGGL(k_bounds_xy, dim3(nb), dim3(kBlock), 0, st, x, y, n, part);
  hipLaunchKernelGGL(k_bounds_xy_final, dim3(1), dim3(kBlock), 0, st, part, nb, d);
  RPT_CHECK_LAUNCH();
  uint32_t h[4];
  RPT_HIP(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  for (int k = 0; k < 4; ++k) out4[k] = ord2f(h[k]);
  return RPT_OK;
}

// the grid's counts and sums (and a caller's 64-bit counter) zeroed in ONE launch: two fills
// and a third for the counter each cost a launch right after the host-synchronous bounds
// readback, when the GPU idles on the host issuing them
__global__ void k_zero_land(int32_t* __restrict__ cnt, double* __restrict__ tot, int64_t cells,
                            int64_t* __restrict__ extra) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells;
       i += (int64_t)gridDim.x * blockDim.x) {
    cnt[i] = 0;
    tot[i] = 0.0;
  }
  if (extra && blockIdx.x == 0 && threadIdx.x == 0) *extra = 0;
}

// land_grid_cells (land.h) for cells of type CT and values of type VT
template <class CT, class VT>
static int32_t land_grid_cells_t(const float* x, const float* y, const VT* val, int64_t n,
                                 const double* xe, int32_t nxe, const double* ye, int32_t nye,
                                 int32_t* cnt, double* tot, CT* cell_out, hipStream_t st,
                                 int32_t u8_vals, int64_t* zero_also) {
  if (nxe < 2 || nye < 2) {
    set_error("rpt_land_grid: need at least two edges per axis");
    return RPT_EINVAL;
  }
  const int64_t cells = (int64_t)(nxe - 1) * (nye - 1);
  if (sizeof(CT) == 4 && cell_out && cells >= (int64_t(1) << 31)) cell_out = nullptr;
  if (sizeof(CT) == 2 && cell_out && cells > 65536) {
    set_error("land_grid_cells: more than 65,536 cells do not fit 16-bit cell ids");
    return RPT_EINVAL;
  }
  hipLaunchKernelGGL(k_zero_land, dim3(grid_for(cells, 256, 1024)), dim3(256), 0, st, cnt, tot,
                     cells, zero_also);
  RPT_CHECK_LAUNCH();
  if (n == 0) return RPT_OK;
  const int64_t ne_al = ((int64_t)nxe + nye + 1) & ~int64_t(1);
  const size_t lds = (size_t)ne_al * 8 + (size_t)cells * 12;
  const size_t lds_u8 = (size_t)ne_al * 8 + (size_t)cells * 8;
  int dev = 0, n_cu = 0;
  RPT_HIP(hipGetDevice(&dev));
  RPT_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  const int gb = grid_for(n, kGridBlock, std::max(n_cu, 1));
  if (u8_vals && lds_u8 <= 150 * 1024 && (n + gb - 1) / gb < (int64_t(1) << 24) &&
      ab().land_u8) {
    RPT_HIP(hipFuncSetAttribute((const void*)k_land_grid_lds_u8<CT, VT>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_u8));
    hipLaunchKernelGGL((k_land_grid_lds_u8<CT, VT>), dim3(gb), dim3(kGridBlock), lds_u8, st, x, y, val, n,
                       xe, nxe, ye, nye, cnt, tot, cell_out);
  } else if (cells <= kLdsGridCells && lds <= 150 * 1024) {
    RPT_HIP(hipFuncSetAttribute((const void*)k_land_grid_lds<CT, VT>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_land_grid_lds<CT, VT>), dim3(gb),
                       dim3(kGridBlock), lds, st, x, y, val, n, xe, nxe, ye, nye, cnt, tot,
                       cell_out);
  } else {
    hipLaunchKernelGGL((k_land_grid<CT, VT>), dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, st, x,
                       y, val, n, xe, nxe, ye, nye, cnt, tot, cell_out);
  }
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t land_grid_cells(const float* x, const float* y, const float* val, int64_t n,
                        const double* xe, int32_t nxe, const double* ye, int32_t nye,
                        int32_t* cnt, double* tot, int32_t* cell_out, hipStream_t st,
                        int32_t u8_vals, int64_t* zero_also, uint16_t* cell16_out,
                        const uint8_t* val8) {
  if (val8 && cell16_out)
    return land_grid_cells_t<uint16_t, uint8_t>(x, y, val8, n, xe, nxe, ye, nye, cnt, tot,
                                                cell16_out, st, 1, zero_also);
  if (val8)
    return land_grid_cells_t<int32_t, uint8_t>(x, y, val8, n, xe, nxe, ye, nye, cnt, tot,
                                               cell_out, st, 1, zero_also);
  if (cell16_out) {
    set_error("land_grid_cells: 16-bit cells come with u8 values");
    return RPT_EINVAL;
  }
  return land_grid_cells_t<int32_t, float>(x, y, val, n, xe, nxe, ye, nye, cnt, tot, cell_out,
                                           st, u8_vals, zero_also);
}

int32_t land_grid(const float* x, const float* y, const float* val, int64_t n, const double* xe,
                  int32_t nxe, const double* ye, int32_t nye, int32_t* cnt, double* tot,
                  hipStream_t st) {
  return land_grid_cells(x, y, val, n, xe, nxe, ye, nye, cnt, tot, nullptr, st, 0, nullptr,
                         nullptr, nullptr);
}

int32_t land_mask_dev(const int32_t* cnt, const double* tot, int64_t cells, int64_t num_frames,
                      double pthr, double ithr, uint8_t* land, int32_t* n_land_dev,
                      hipStream_t st) {
  const double nf = (double)(num_frames > 1 ? num_frames : 1);
  if (cells > 0) {
    hipLaunchKernelGGL(k_land_mask, dim3(grid_for(cells, 256, 1024)), dim3(256), 0, st, cnt, tot,
                       cells, nf, pthr, ithr, land, n_land_dev);
    RPT_CHECK_LAUNCH();
  }
  return RPT_OK;
}

int32_t land_mask(const int32_t* cnt, const double* tot, int64_t cells, int64_t num_frames,
                  double pthr, double ithr, uint8_t* land, int64_t* n_land_host,
                  hipStream_t st) {
  int32_t* d = nullptr;
  RPT_TRY(zero_n(st, 1, &d));
  RPT_TRY(land_mask_dev(cnt, tot, cells, num_frames, pthr, ithr, land, d, st));
  if (n_land_host) {
    int32_t h = 0;
    RPT_HIP(hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
    *n_land_host = h;
  }
  return RPT_OK;
}

int32_t land_filter(const float* x, const float* y, const float* v, const int32_t* g,
                    const int32_t* pf, int64_t n, const int64_t* frame_off, int32_t n_frames,
                    const double* xe, int32_t nxe, const double* ye, int32_t nye,
                    const uint8_t* land, float* xo, float* yo, float* vo, int32_t* go,
                    int32_t* pfo, int64_t* new_off, int64_t* n_kept_host, hipStream_t st) {
  Scratch& sc = scratch(st);
  if (n >= (int64_t(1) << 31) - 1) {
    set_error("rpt_land_filter: n exceeds the int32 index space");
    return RPT_ENOTSUP;
  }
  Budget b;
  b.add<int32_t>(n + 1);
  b.add<int32_t>(n + 1);
  RPT_TRY(sc.reserve(b.bytes, st));
  int32_t* keep = sc.carve_n<int32_t>(n + 1);
  int32_t* pos = sc.carve_n<int32_t>(n + 1);  // int32 kept positions (n < 2^31)
  if (n > 0) {
    hipLaunchKernelGGL(k_land_keep, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, st, x, y,
                       n, xe, nxe, ye, nye, land, keep);
    RPT_CHECK_LAUNCH();
  }
  RPT_TRY(exclusive_scan_total_i32(keep, pos, n, st));
  if (n > 0) {
    hipLaunchKernelGGL(k_land_scatter, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, st, x,
                       y, v, g, pf, n, keep, pos, xo, yo, vo, go, pfo);
    RPT_CHECK_LAUNCH();
  }
  if (new_off && frame_off) {
    hipLaunchKernelGGL(k_new_offsets, dim3(grid_for(n_frames + 1, 256, 64)), dim3(256), 0, st,
                       pos, frame_off, n_frames, new_off);
    RPT_CHECK_LAUNCH();
  }
  if (n_kept_host) {
    int32_t k = 0;
    RPT_HIP(hipMemcpyAsync(&k, pos + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
    *n_kept_host = k;
  }
  return RPT_OK;
}

int32_t land_compact_dev(const float* x, const float* y, const float* v, const int32_t* g,
                         const int32_t* pf, int64_t n, const int32_t* cell, const uint8_t* land,
                         int32_t n_frames, float* xo, float* yo, float* vo, int32_t* go,
                         int32_t* pfo, float* to, int64_t* new_off, Bounds* bounds_out,
                         hipStream_t st, int64_t t_base, const int64_t* frame_off,
                         const uint16_t* cell16, const uint8_t* v8, uint8_t* vo8) {
  if ((frame_off != nullptr) != (v8 && vo8) || (cell16 && !frame_off)) {
    set_error("land_compact_dev: frame offsets, u8 intensities and 16-bit cells come together");
    return RPT_EINVAL;
  }
  if (n < 0 || n >= (int64_t(1) << 31) - 1 || n_frames < 0) {
    set_error("land_compact_dev: bad sizes");
    return RPT_EINVAL;
  }
  const int64_t nt = std::max<int64_t>((n + kCompTile - 1) / kCompTile, 1);
  Scratch& sc = scratch(st);
  Budget bud;
  bud.add<int32_t>(nt + 1);
  bud.add<int32_t>(nt + 1);
  bud.add<BoundsPart>(nt);
  RPT_TRY(sc.reserve(bud.bytes, st));
  int32_t* cnt = sc.carve_n<int32_t>(nt + 1);
  int32_t* base = sc.carve_n<int32_t>(nt + 1);
  BoundsPart* part = sc.carve_n<BoundsPart>(nt);
  if (cell16)
    hipLaunchKernelGGL(k_land_tile_counts<uint16_t>, dim3((unsigned)nt), dim3(kCompBlock), 0, st,
                       cell16, n, land, cnt);
  else
    hipLaunchKernelGGL(k_land_tile_counts<int32_t>, dim3((unsigned)nt), dim3(kCompBlock), 0, st,
                       cell, n, land, cnt);
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i32(cnt, base, nt, st));
  if (frame_off && n > 0 && cell16) {
    hipLaunchKernelGGL((k_land_compact<true, uint16_t, uint8_t>), dim3((unsigned)nt),
                       dim3(kCompBlock), 0, st, x, y, v8, g, nullptr, n, cell16, land, base, xo,
                       yo, vo8, go, nullptr, to, part, t_base, frame_off, n_frames);
    hipLaunchKernelGGL(k_land_new_off_tiles<uint16_t>, dim3(n_frames + 1), dim3(kCompBlock), 0,
                       st, base, cell16, land, frame_off, new_off);
  } else if (frame_off && n > 0) {
    hipLaunchKernelGGL((k_land_compact<true, int32_t, uint8_t>), dim3((unsigned)nt),
                       dim3(kCompBlock), 0, st, x, y, v8, g, nullptr, n, cell, land, base, xo, yo,
                       vo8, go, nullptr, to, part, t_base, frame_off, n_frames);
    hipLaunchKernelGGL(k_land_new_off_tiles<int32_t>, dim3(n_frames + 1), dim3(kCompBlock), 0,
                       st, base, cell, land, frame_off, new_off);
  } else {
    hipLaunchKernelGGL((k_land_compact<false, int32_t, float>), dim3((unsigned)nt), dim3(kCompBlock), 0, st, x, y,
                       v, g, pf, n, cell, land, base, xo, yo, vo, go, pfo, to, part, t_base,
                       nullptr, 0);
    hipLaunchKernelGGL(k_land_new_off, dim3((n_frames + 1 + 3) / 4), dim3(256), 0, st, base + nt,
                       pfo, n_frames, new_off);
  }
  hipLaunchKernelGGL(k_land_compact_final, dim3(1), dim3(kFinBlock), 0, st, part, (int)nt,
                     base + nt, bounds_out, t_base);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

}  // namespace rpt
