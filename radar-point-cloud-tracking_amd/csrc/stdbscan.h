// The rpt:: functions that stdbscan.hip defines, declared once.  Included by stdbscan.hip itself,
// so every definition is compiled against its declaration, by abi.cpp (the extern "C" surface)
// and by stack_impl.h (the stack and shard drivers).
#pragma once
#include "common.h"

namespace rpt {

// ---- the fused entry points
// labels[n]; z (with its stride) and dim 3 for 3-D points, otherwise z is not read
int32_t stdbscan(const float* x, const float* y, const float* z, int64_t stride, const float* t,
                 int64_t n, double eps_space, double eps_time, int32_t min_samples,
                 int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st, int dim);
// counts[n] (original order): the exact neighbour counts of stdbscan's neighbour test, the point
// itself included (stdbscan_count.inc)
int32_t neighbour_counts(const float* x, const float* y, const float* z, int64_t stride,
                         const float* t, int64_t n, double eps_space, double eps_time,
                         int32_t* counts, hipStream_t st, int dim);
// stdbscan for n_sets values of min_samples (host, each >= 1) from one bounds pass, grid build and
// count pass: labels[n_sets][n], counts[n] (nullable), stats[n_sets] (nullable)
int32_t stdbscan_sweep(const float* x, const float* y, const float* z, int64_t stride,
                       const float* t, int64_t n, double eps_space, double eps_time,
                       const int32_t* min_samples, int32_t n_sets, int32_t* counts,
                       int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st, int dim);
// Denoise variant (PointCloudWorkF/stdbscan_denoising_pipeline.py:264-369), 2-D.
int32_t stdbscan_denoise(const float* x, const float* y, const float* t, int64_t n,
                         double eps_space, double eps_time, int32_t min_samples,
                         int32_t min_frames, int32_t* labels, rpt_stdbscan_stats* stats,
                         hipStream_t st);
// The fused path without its readbacks (the native stack driver): the cluster count stays on the
// device at *n_clusters_dev (nullptr when the parameters are degenerate: stats is then complete)
// and stdbscan_fill_stats completes stats after the caller has synchronised the stream.
// *state: the stream's state, for stdbscan_fill_stats and stdbscan_core_flags.  host_bounds
// (nullable): the points' Bounds, read back by the caller already (no bounds pass).
int32_t stdbscan_deferred(const float* x, const float* y, const float* z, int64_t stride,
                          const float* t, int64_t n, double eps_space, double eps_time,
                          int32_t min_samples, int32_t* labels, rpt_stdbscan_stats* stats,
                          hipStream_t st, int dim, const int32_t** n_clusters_dev,
                          void** state, const void* host_bounds);
int32_t stdbscan_fill_stats(void* state, int32_t n_clusters, rpt_stdbscan_stats* stats);
// core flags (original order) of the state's last run: the stack driver's K5 result, for tests
int32_t stdbscan_core_flags(void* state, int64_t n, uint8_t* out, hipStream_t st);

// ---- bounds for a caller that reads them back together with its own results
// Bounds of the 2-D points [0, *n_dev) (n_dev on the device, <= n_max) into out_dev
// (stdbscan_bounds_bytes(), device): what stdbscan_deferred's build would compute.  part_dev:
// stdbscan_bounds_part_bytes(n_max) bytes.
size_t stdbscan_bounds_bytes();
// the partials of a bounds pass of kBoundsBlock-thread blocks (k_bounds, or k_window in the
// shard driver) over at most n_max points: one per block of grid_for(n_max, kBoundsBlock, 1024)
size_t stdbscan_bounds_part_bytes(int64_t n_max);
int32_t stdbscan_bounds_dev(const float* x, const float* y, const float* t, int64_t n_max,
                            const int64_t* n_dev, void* out_dev, void* part_dev, hipStream_t st);
// the partials of nb blocks -> out (one launch, k_bounds_final; see BoundsAcc, common.h)
int32_t stdbscan_bounds_final_dev(const void* part_dev, int nb, void* out_dev, hipStream_t st);

// ---- the phased bodies (rpt_dbscan_*: the distributed driver runs its collectives between them)
struct DbscanState;
DbscanState* dbscan_create();
void dbscan_destroy(DbscanState* s);
int32_t dbscan_build(DbscanState* S, const float* x, const float* y, const float* z,
                     int64_t stride, const float* t, int64_t n, double eps_space,
                     double eps_time, int32_t ms, hipStream_t st);
// core_out (nullable): the core flags in original order
int32_t dbscan_core(DbscanState* S, uint8_t* core_out, hipStream_t st);
int32_t dbscan_set_core(DbscanState* S, const uint8_t* core_in, hipStream_t st);
int32_t dbscan_components(DbscanState* S, int32_t* comp_out, hipStream_t st);
int32_t dbscan_labels_global(DbscanState* S, const int64_t* rep, const int64_t* reps, int64_t nr,
                             int32_t* labels, hipStream_t st);

// ---- the frame-sharded driver's forms (shard.cpp)
// grid bounds read back by the caller with its own results (host_bounds: a Bounds)
int32_t dbscan_build_given(DbscanState* S, const float* x, const float* y, const float* t,
                           int64_t n, double eps_space, double eps_time, int32_t ms,
                           const void* host_bounds, hipStream_t st);
// the representative count on the device (nr_dev)
int32_t dbscan_labels_global_dev(DbscanState* S, const int64_t* rep, const int64_t* reps,
                                 const int64_t* nr_dev, int32_t* labels, hipStream_t st);
// the core flags in original order
int32_t dbscan_core_orig(DbscanState* S, uint8_t* out, hipStream_t st);
// the component ids (as dbscan_components) of the original indices outside [lo_end, hi_begin)
int32_t dbscan_components_edges(DbscanState* S, int32_t* comp_out, int64_t lo_end,
                                int64_t hi_begin, hipStream_t st);
// the union-find state for the shard driver's per-root passes: a core point s is its
// component's root iff parent[s] == s (the component's minimum original index is sorig[s])
void dbscan_uf_arrays(const DbscanState* S, const uint8_t** core, const int32_t** parent,
                      const int32_t** sorig, int64_t* n);
// the edge forms of dbscan_core / dbscan_set_core: core flags of the original indices [a0, a1)
// -> out_a and [b0, b1) -> out_b (the own edge frames, for the neighbours), and the halo points'
// flags from their owners (original indices [0, a1) <- in_a, [b0, n) <- in_b): one coalesced
// index read per sorted point instead of full-length scattered conversions both ways around the
// halo update
int32_t dbscan_core_edges(DbscanState* S, int64_t a0, int64_t a1, uint8_t* out_a, int64_t b0,
                          int64_t b1, uint8_t* out_b, hipStream_t st);
int32_t dbscan_set_core_edges(DbscanState* S, const uint8_t* in_a, int64_t a1,
                              const uint8_t* in_b, int64_t b0, hipStream_t st);

}  // namespace rpt
