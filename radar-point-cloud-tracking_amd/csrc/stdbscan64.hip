// ST-DBSCAN on float64 coordinates for gfx950 (rpt_stdbscan_f64): the general entry point for
// inputs that float32 cannot hold -- decimal CSV columns, projected coordinates with large
// offsets, epoch times.  The contract is in stdbscan64.h; the float32 unit (stdbscan.hip) and
// every input that takes it are untouched by this one.
//
// Plain by design: a uniform grid whose cell side is eps (so a neighbour is within +-1 cell,
// grid64.h), the points sorted by cell, and three passes that walk each point's window with the
// exact pair test -- no per-cell screens.  Stage files, included inside namespace rpt {
// namespace { in this order; each reads stdbscan64_shared.inc and the stages before it:
//   stdbscan64_shared.inc  launch geometry, Geom64, the pair test, the window walk (no kernel)
//   stdbscan64_grid.inc    bounds, keys, sorted points, cell starts
//   stdbscan64_core.inc    core flags
//   stdbscan64_union.inc   core-core components (lock-free union-find)
//   stdbscan64_label.inc   cluster ids and labels
// The unit reads no A/B switch.
#include <climits>
#include <cmath>

#include "common.h"
#include "grid64.h"
#include "stdbscan64.h"

#pragma clang fp contract(off)

namespace rpt {

namespace {

#include "stdbscan64_shared.inc"
#include "stdbscan64_grid.inc"
#include "stdbscan64_core.inc"
#include "stdbscan64_union.inc"
#include "stdbscan64_label.inc"

// hipEvent marks between the stages, created only for a timed call
struct StageTimer {
  bool on = false;
  hipStream_t st{};
  hipEvent_t ev[6]{};
  int k = 0;
  void start(bool enable, hipStream_t s) {
    on = enable;
    st = s;
    if (!on) return;
    for (auto& e : ev) (void)hipEventCreate(&e);
    mark();
  }
  void mark() {
    if (on && k < 6) (void)hipEventRecord(ev[k++], st);
  }
  double ms(int i) {
    float t = 0;
    (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
    return t;
  }
  ~StageTimer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int32_t check_args(const double* x, const double* y, const double* z, int64_t stride,
                   const void* t, int32_t time_dtype, int64_t n, const int32_t* labels) {
  if (n <= 0) {
    set_error("Found array with 0 sample(s) (shape=(0, %d)) while a minimum of 1 is required.",
              z ? 3 : 2);
    return RPT_EEMPTY;
  }
  if (n >= (int64_t(1) << 31) - 2) {
    set_error("rpt_stdbscan_f64: n=%lld exceeds the int32 index space", (long long)n);
    return RPT_ENOTSUP;
  }
  if (!x || !y || !t || !labels || stride < 1) {
    set_error("rpt_stdbscan_f64: null pointer or bad stride");
    return RPT_EINVAL;
  }
  if (time_dtype != RPT_TIME_F32 && time_dtype != RPT_TIME_F64) {
    set_error("rpt_stdbscan_f64: time_dtype must be RPT_TIME_F32 or RPT_TIME_F64");
    return RPT_EINVAL;
  }
  return RPT_OK;
}

template <int D, bool TF64>
int32_t run(const double* x, const double* y, const double* z, int64_t stride, const void* t,
            int64_t n64, double eps_space, double eps_time, int32_t min_samples, int32_t* labels,
            rpt_stdbscan_stats* stats, hipStream_t st) {
  const int32_t n = (int32_t)n64;
  StageTimer tm;
  tm.start(stats && stats->timing, st);
  const int gp = grid_for(n, kBlock, kCapPoint);
  const int gw = grid_for(n, kPtsPerBlock, kCapWalk);
  const int nbb = grid_for(n, kBlock, kCapBounds);
  // ---- the one reservation: the cell count is not known before the bounds are, so the cells'
  // array is sized by the cell cap
  const int64_t cmax = grid64_cell_cap(n);
  Scratch& arena = scratch(st);
  Budget bud;
  bud.add<Bounds64>(1);
  bud.add<Bounds64>(nbb);
  for (int k = 0; k < 4; ++k) bud.add<uint32_t>(n);  // keys, vals and their alternates
  bud.add<int64_t>(radix_tmp_elems(n));
  for (int k = 0; k < 4; ++k) bud.add<double>(n);  // sorted x, y, z, t
  bud.add<int32_t>(n);                             // sorig
  bud.add<int32_t>(n);                             // skey
  bud.add<int32_t>(cmax + 2);                      // cell_start
  bud.add<uint8_t>(n);                             // core
  bud.add<int32_t>(n);                             // parent
  bud.add<int32_t>(n + 1);                         // is_root / rank (+ the cluster count)
  bud.add<int32_t>(n);                             // cid
  RPT_TRY(arena.reserve(bud.bytes, st));
  Bounds64* d_b = arena.carve_n<Bounds64>(1);
  Bounds64* d_part = arena.carve_n<Bounds64>(nbb);
  uint32_t* keys = arena.carve_n<uint32_t>(n);
  uint32_t* vals = arena.carve_n<uint32_t>(n);
  uint32_t* keys_alt = arena.carve_n<uint32_t>(n);
  uint32_t* vals_alt = arena.carve_n<uint32_t>(n);
  int64_t* rtmp = arena.carve_n<int64_t>(radix_tmp_elems(n));
  double* sx = arena.carve_n<double>(n);
  double* sy = arena.carve_n<double>(n);
  double* sz = arena.carve_n<double>(n);
  double* stime = arena.carve_n<double>(n);
  int32_t* sorig = arena.carve_n<int32_t>(n);
  int32_t* skey = arena.carve_n<int32_t>(n);
  int32_t* cell_start = arena.carve_n<int32_t>(cmax + 2);
  uint8_t* core = arena.carve_n<uint8_t>(n);
  int32_t* parent = arena.carve_n<int32_t>(n);
  int32_t* rank = arena.carve_n<int32_t>(n + 1);
  int32_t* cid = arena.carve_n<int32_t>(n);
  if (!d_b || !cid) {
    set_error("internal: scratch carve overflow");
    return RPT_ENOMEM;
  }
  // ---- bounds (the first sync)
  hipLaunchKernelGGL(k64_bounds<D>, dim3(nbb), dim3(kBlock), 0, st, x, y, z, stride, t, TF64,
                     n64, d_part);
  hipLaunchKernelGGL(k64_bounds_final, dim3(1), dim3(kBlock), 0, st, d_part, nbb, d_b);
  RPT_CHECK_LAUNCH();
  Bounds64 hb;
  RPT_HIP(hipMemcpyAsync(&hb, d_b, sizeof(Bounds64), hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  tm.mark();
  if (hb.nonfinite_xyz) {
    set_error("Input contains NaN or infinity in coordinates");
    return RPT_ENONFINITE;
  }
  // ---- geometry (grid64.h)
  const float epst32 = (float)eps_time;
  const Grid64 gr = grid64_plan(hb.mn, hb.mx, hb.n_finite_t, D, eps_space,
                                TF64 ? eps_time : (double)epst32, n);
  if (gr.cells > cmax) {
    set_error("internal: grid64_plan exceeded the cell cap");
    return RPT_EHIP;
  }
  Geom64 g{};
  g.ox = gr.lo[0];
  g.oy = gr.lo[1];
  g.oz = gr.lo[2];
  g.ot = gr.lo[3];
  g.cs = gr.cs;
  g.ct = gr.ct;
  g.eps2 = eps_space * eps_space;
  g.epst = eps_time;
  g.epst32 = epst32;
  g.nx = gr.nx;
  g.ny = gr.ny;
  g.nz = gr.nz;
  g.nt = gr.nt;
  g.cells = (int32_t)gr.cells;
  g.min_samples = min_samples;
  const int64_t C1 = gr.cells + 1;  // + the isolated cell
  // ---- sort by cell
  hipLaunchKernelGGL(k64_keys<D>, dim3(gp), dim3(kBlock), 0, st, x, y, z, stride, t, TF64, n64, g,
                     keys, vals);
  RPT_CHECK_LAUNCH();
  int bits = 1;
  while ((int64_t(1) << bits) < C1) ++bits;  // keys are in [0, C1)
  uint32_t *sk, *sv;
  RPT_TRY(radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, bits, rtmp, &sk, &sv, st));
  hipLaunchKernelGGL(k64_gather<D>, dim3(gp), dim3(kBlock), 0, st, x, y, z, stride, t, TF64, n64,
                     sk, sv, sx, sy, sz, stime, sorig, skey);
  hipLaunchKernelGGL(k64_cell_start, dim3(grid_for(C1 + 1, kBlock, kCapCell)), dim3(kBlock), 0,
                     st, skey, n, C1, cell_start);
  RPT_CHECK_LAUNCH();
  tm.mark();
  const Pts64 p{sx, sy, D == 3 ? sz : nullptr, stime};
  // ---- core flags
  hipLaunchKernelGGL((k64_core<D, TF64>), dim3(gw), dim3(kBlock), 0, st, p, g, cell_start, skey,
                     n, core);
  RPT_CHECK_LAUNCH();
  tm.mark();
  // ---- components
  hipLaunchKernelGGL(k64_parent_init, dim3(gp), dim3(kBlock), 0, st, parent, n);
  hipLaunchKernelGGL((k64_union<D, TF64>), dim3(gw), dim3(kBlock), 0, st, p, g, cell_start, skey,
                     sorig, core, n, parent);
  RPT_CHECK_LAUNCH();
  tm.mark();
  // ---- ids and labels (the second sync: the cluster count)
  hipLaunchKernelGGL(k64_roots, dim3(gp), dim3(kBlock), 0, st, sorig, core, parent, n, rank);
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i32(rank, rank, n, st));
  hipLaunchKernelGGL(k64_cid, dim3(gp), dim3(kBlock), 0, st, sorig, core, parent, rank, n, cid);
  hipLaunchKernelGGL((k64_label<D, TF64>), dim3(gw), dim3(kBlock), 0, st, p, g, cell_start, skey,
                     sorig, cid, n, labels);
  RPT_CHECK_LAUNCH();
  tm.mark();
  if (!stats) return RPT_OK;
  int32_t ncl = 0;
  RPT_HIP(hipMemcpyAsync(&ncl, rank + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  stats->n_points = n;
  stats->n_clusters = ncl;
  stats->n_core = -1;
  stats->grid_dims[0] = g.nx;
  stats->grid_dims[1] = g.ny;
  stats->grid_dims[2] = g.nz;
  stats->grid_dims[3] = g.nt;
  stats->grid_cells = gr.cells;
  if (tm.on && tm.k == 6) {
    RPT_HIP(hipEventSynchronize(tm.ev[5]));
    stats->ms_bounds = tm.ms(0);
    stats->ms_grid = tm.ms(1);
    stats->ms_core = tm.ms(2);
    stats->ms_union = tm.ms(3);
    stats->ms_label = tm.ms(4);
  }
  return RPT_OK;
}

}  // namespace

int32_t stdbscan_f64(const double* x, const double* y, const double* z, int64_t stride,
                     const void* times, int32_t time_dtype, int64_t n, double eps_space,
                     double eps_time, int32_t min_samples, int32_t* labels,
                     rpt_stdbscan_stats* stats, hipStream_t st) {
  RPT_TRY(check_args(x, y, z, stride, times, time_dtype, n, labels));
  const bool tf64 = time_dtype == RPT_TIME_F64;
  // negative or NaN eps: no pair passes, not even (i, i)
  const bool degenerate =
      !(eps_space >= 0.0) || (tf64 ? !(eps_time >= 0.0) : !((float)eps_time >= 0.0f));
  if (degenerate) {
    hipLaunchKernelGGL(k64_fill, dim3(grid_for(n, kBlock, kCapPoint)), dim3(kBlock), 0, st,
                       labels, (int32_t)n, min_samples <= 0);
    RPT_CHECK_LAUNCH();
    if (stats) {
      stats->n_points = n;
      stats->n_core = min_samples <= 0 ? n : 0;
      stats->n_clusters = min_samples <= 0 ? (int32_t)n : 0;
    }
    return RPT_OK;
  }
  if (z)
    return tf64 ? run<3, true>(x, y, z, stride, times, n, eps_space, eps_time, min_samples,
                               labels, stats, st)
                : run<3, false>(x, y, z, stride, times, n, eps_space, eps_time, min_samples,
                                labels, stats, st);
  return tf64 ? run<2, true>(x, y, z, stride, times, n, eps_space, eps_time, min_samples, labels,
                             stats, st)
              : run<2, false>(x, y, z, stride, times, n, eps_space, eps_time, min_samples,
                              labels, stats, st);
}

}  // namespace rpt
