// The rpt:: functions that stdbscan64.hip defines, declared once.  Included by stdbscan64.hip
// itself and by abi.cpp (the extern "C" surface).
//
// ST-DBSCAN on float64 coordinates: rpt_stdbscan's contract (stdbscan.hip) with double
// coordinates and a choice of time dtype.
//   nbr(i,j)  <=>  d2(i,j) <= eps_space^2   float64 d2 = ((xi-xj)^2 + (yi-yj)^2) [+ (zi-zj)^2],
//                  each operation rounded, no FMA
//             and  RPT_TIME_F32: |f32(t_j - t_i)| <= f32(eps_time)
//                  RPT_TIME_F64: float64 |t_j - t_i| <= eps_time
//   a point with a NaN or infinite time is nobody's neighbour, not even its own (inf - inf = NaN)
//   core(i)   <=>  |{ j : nbr(i,j) }| >= min_samples   (the count includes i itself)
//   clusters  =    components of the core-core graph, numbered in ascending order of each
//                  component's minimum core index
//   border    =    non-core point with a core neighbour: the minimum adjacent cluster id
//   noise     =    -1
// Errors as rpt_stdbscan: non-finite coordinates RPT_ENONFINITE (sklearn's message), n <= 0
// RPT_EEMPTY, n >= 2^31 - 2 RPT_ENOTSUP, a null pointer, a bad stride or an unknown time dtype
// RPT_EINVAL.  Negative or NaN eps_space / eps_time (eps_time tested in double for float64
// times, as float32 for float32 times): no pair passes, so every point is noise, or its own
// cluster when min_samples <= 0; the coordinates are not read then.
// Two syncs: the bounds and the cluster count.  All device memory is one reservation of the
// (device, stream) scratch arena, made before the first launch.
#pragma once
#include "common.h"

namespace rpt {

// x, y, z: device doubles, `stride` elements between consecutive points (z null: 2-D); times:
// n contiguous device floats (RPT_TIME_F32) or doubles (RPT_TIME_F64); labels: device int32 [n]
int32_t stdbscan_f64(const double* x, const double* y, const double* z, int64_t stride,
                     const void* times, int32_t time_dtype, int64_t n, double eps_space,
                     double eps_time, int32_t min_samples, int32_t* labels,
                     rpt_stdbscan_stats* stats, hipStream_t st);

}  // namespace rpt
