// The rpt:: functions that land.hip defines, declared once (default arguments only here).
// Included by land.hip itself, so every definition is compiled against its declaration, by
// abi.cpp (the extern "C" surface), by stack_impl.h (the stack and shard drivers) and by
// fusion.hip (bounds_xy).
#pragma once
#include "common.h"

namespace rpt {

// out4 (host): min x, max x, min y, max y of the points [0, n), n > 0.  Synchronises.
int32_t bounds_xy(const float* x, const float* y, int64_t n, float* out4, hipStream_t st);

// ---- K2: occupancy grid and land mask
// cnt / tot ([(nxe - 1) * (nye - 1)], zeroed here): per-cell point counts and intensity sums over
// the edges xe / ye (device, float64).
// cell_out (nullable, [n], int32 cells < 2^31): each point's grid cell, for land_compact_dev
// u8_vals: every val is an integer in [0, 255] (points of a u8 echo; packed-atomic kernel)
// zero_also (nullable): a 64-bit device counter zeroed with the grid
// cell16_out (nullable; grids of at most 65,536 cells): the per-point cells as uint16_t instead
// of cell_out; val8 (nullable): the values as uint8_t samples instead of val (u8_vals holds by
// construction) -- both the stack driver's narrow path
int32_t land_grid_cells(const float* x, const float* y, const float* val, int64_t n,
                        const double* xe, int32_t nxe, const double* ye, int32_t nye,
                        int32_t* cnt, double* tot, int32_t* cell_out, hipStream_t st,
                        int32_t u8_vals, int64_t* zero_also = nullptr,
                        uint16_t* cell16_out = nullptr, const uint8_t* val8 = nullptr);
// land_grid_cells without stored cells, float values
int32_t land_grid(const float* x, const float* y, const float* val, int64_t n, const double* xe,
                  int32_t nxe, const double* ye, int32_t nye, int32_t* cnt, double* tot,
                  hipStream_t st);
// land[cell] = 1 where count / num_frames >= pthr and the mean intensity >= ithr.
// n_land_dev: int32 land-cell counter on the device, zeroed by the caller (no readback)
int32_t land_mask_dev(const int32_t* cnt, const double* tot, int64_t cells, int64_t num_frames,
                      double pthr, double ithr, uint8_t* land, int32_t* n_land_dev,
                      hipStream_t st);
// land_mask_dev with a counter of its own, read back into *n_land_host (nullable: no readback)
int32_t land_mask(const int32_t* cnt, const double* tot, int64_t cells, int64_t num_frames,
                  double pthr, double ithr, uint8_t* land, int64_t* n_land_host,
                  hipStream_t st);

// ---- K3: the points outside land cells
// The public call's filter: the kept points of [0, n) in order into xo / yo / vo / go (nullable)
// / pfo (nullable), cells searched in the edges.  new_off (nullable, with frame_off; device,
// [n_frames + 1]): the kept points' frame offsets.  *n_kept_host (nullable): the kept count,
// read back.
int32_t land_filter(const float* x, const float* y, const float* v, const int32_t* g,
                    const int32_t* pf, int64_t n, const int64_t* frame_off, int32_t n_frames,
                    const double* xe, int32_t nxe, const double* ye, int32_t nye,
                    const uint8_t* land, float* xo, float* yo, float* vo, int32_t* go,
                    int32_t* pfo, int64_t* new_off, int64_t* n_kept_host, hipStream_t st);
// The stack driver's land compaction (see k_land_compact): kept points of [0, n) -- cells from
// land_grid_cells, land flags from land_mask_dev -- into xo / yo / vo / go (nullable) / pfo and
// their times to (float32 frame slot), new_off[n_frames + 1] (device: first kept point per
// frame slot, kept count last) and the kept points' ST-DBSCAN bounds (*bounds_out, device).
// pf must be non-decreasing (the stack's frame-major order).  No synchronisation.
// frame_off (nullable; device, [n_frames + 1], frame_off[n_frames] = n): the input's frame
// offsets instead of pf; then pf and pfo are not touched (the stack driver's narrow path).
// cell16 (nullable, with frame_off only): the cells as uint16_t instead of cell.
// v8, vo8 (with frame_off, and only then): the intensities as uint8_t samples instead of v, vo.
int32_t land_compact_dev(const float* x, const float* y, const float* v, const int32_t* g,
                         const int32_t* pf, int64_t n, const int32_t* cell, const uint8_t* land,
                         int32_t n_frames, float* xo, float* yo, float* vo, int32_t* go,
                         int32_t* pfo, float* to, int64_t* new_off, Bounds* bounds_out,
                         hipStream_t st, int64_t t_base = 0,
                         const int64_t* frame_off = nullptr, const uint16_t* cell16 = nullptr,
                         const uint8_t* v8 = nullptr, uint8_t* vo8 = nullptr);

}  // namespace rpt
