// Frame-sharded multi-GPU driver: one rank's phases of ONE global stack whose
// contiguous frame ranges are spread over ranks (4_temporal_object_tracker.py:466-506 clusters the
// whole stack at once; the result here is identical to rpt_stack_run over the whole stack).
//
// The caller (rpt/dist.py: torch.distributed over RCCL, or gloo) runs the collectives between the
// phases on buffers it owns.  Only three points of a step wait on the host:
//
//   polar   K1 + xy bounds + the K1 counts of the edge frames          (readback 1)
//     [all_gather info]                                                (host: land edges, caps)
//   land    land grid over the global edges
//     [all_reduce grid]                                                (device)
//   halo    land mask + compaction, the own edge frames packed for the neighbours
//     [P2P x/y/t, capacity = the neighbour's K1 edge count]            (device)
//   window  [prev halo | own | next halo] assembled, bounds            (readback 2)
//           grid build (host-sized) + core flags, own edge flags packed
//     [P2P core flags]                                                 (device)
//   link    halo flags from their owners, components, own edge component ids packed
//     [P2P component ids]                                              (device)
//   pairs   distinct (my id, owner's id) pairs of the halo points
//     [all_gather pairs, capacity]                                     (device)
//   finish  equivalence merge on the device (every rank the same), representatives, labels,
//           K9 of the own points, everything rank 0 needs packed
//     [all_gather packed results, capacity]                            (readback 3)
//
// Point ids are (rank << 40) | own index, so no rank needs another rank's point count to number
// its points, and id order is the global point order (frames are in rank order).  Labels are
// numbered per rank (dense over the representatives its window sees, in id order) and mapped to
// the global numbering on rank 0, which has every rank's representative table: the numbering
// preserves order, so every "smallest adjacent cluster" decision is the global one.
#include "shard_pack.h"
#include "stack_impl.h"

namespace rpt {
namespace {

// The kernels by stage; each file's header names the phase that launches them, their order and
// their arrays, and each reads shard_shared.inc and no other stage file.
#include "shard_shared.inc"
#include "shard_bounds.inc"
#include "shard_window.inc"
#include "shard_pairs.inc"
#include "shard_merge.inc"
#include "shard_finish.inc"

}  // namespace
}  // namespace rpt

using namespace rpt;

struct rpt_shard {
  rpt_stack st;                  // K1 / land buffers of the stack driver
  rpt::DbscanState* db = nullptr;
  DevBuf<uint32_t> bnd;          // xy bounds (ordered u32)
  DevBuf<float> X, Y, T;         // the window
  // core flags of the window in original order: filled on demand by rpt_shard_points (checks)
  mutable DevBuf<uint8_t> core;
  DevBuf<int32_t> comp, labels, flag;
  DevBuf<int64_t> rep, reps, keys, vals, pos, cnt64, meta;
  DevBuf<unsigned long long> pset;  // distinct-pair hash set
  DevBuf<char> wbnd;             // window meta + bounds (+ partials)
  rpt_stack_params p{};
  int64_t n_points = 0, frame0 = 0;
  int32_t F = 0, G = 0, hf = 0, rank = 0;
  rpt_shard_info info{};
  int64_t n_window = 0, k_prev_total = 0;
  // direct window (land filter on): the compaction wrote the own kept points' x / y / t into
  // X / Y / T at own_off (= the prev halo's capacity); the window then starts at win_base =
  // own_off - n_prev.  Otherwise the window is assembled from the K1 points at 0.
  bool direct = false;
  int64_t own_off = 0, own_cap_next = 0, win_base = 0;
  bool land = false;
  bool k9_radix = false;
  int32_t merge_max = kMergeMax;  // ids the device merge takes (rpt_shard_set_merge_limit)
  hipEvent_t ev[2] = {};         // around the core-flag pass (params.timing)
  bool ev_ok = false, core_timed = false;
  ~rpt_shard() {  // (the buffers free themselves)
    if (ev_ok)
      for (auto& e : ev) (void)hipEventDestroy(e);
    if (db) rpt::dbscan_destroy(db);
  }
  WinIds ids() const { return WinIds{rank, info.n_prev, info.n_kept, k_prev_total}; }
  // the own kept points' x / y (after the land filter, if any)
  const float* own_x() const { return direct ? X.p + own_off : (st.land_applied ? st.x2.p : st.x.p); }
  const float* own_y() const { return direct ? Y.p + own_off : (st.land_applied ? st.y2.p : st.y.p); }
  // ... and their intensities and frame slots
  const float* own_v() const { return st.land_applied ? st.v2.p : st.v.p; }
  const int32_t* own_pf() const { return st.land_applied ? st.pf2.p : st.pf.p; }
};

extern "C" {

rpt_shard* rpt_shard_create(void) {
  rpt_shard* h = new rpt_shard();
  h->db = dbscan_create();
  return h;
}

void rpt_shard_destroy(rpt_shard* h) { delete h; }

int32_t rpt_shard_polar(rpt_shard* h, const rpt_stack_params* p, const void* echo,
                        const float* scale, const float* cos_t, const float* sin_t,
                        const int32_t* gain, rpt_shard_info* info, void* stream) {
  clear_error();
  if (!h || !p || !info || !echo || !scale || !cos_t || !sin_t || p->n_frames < 0 ||
      p->files_per_frame < 1 || p->rows <= 0 || p->bins <= 0 || p->stride < 1) {
    set_error("rpt_shard_polar: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  RPT_TRY(zero_pool_arm(st));  // the step's counters (this call and the step's later ones)
  rpt_stack& S = h->st;
  h->p = *p;
  S.had_gain = gain != nullptr;  // per-point gains only with a gain table
  const int32_t F = p->n_frames, G = p->files_per_frame;
  h->F = F;
  h->G = G;
  // halo depth: floor(eps_time) frames (a neighbour is at most that many frames away)
  const double et = p->eps_time;
  h->hf = (std::isfinite(et) && et >= 0.0) ? (int32_t)std::min<double>(std::floor(et), F) : 0;
  const int64_t n_files = (int64_t)F * G;
  RPT_TRY(S.file_off.ensure((size_t)n_files + 1, st));
  RPT_TRY(S.row_prefix.ensure((size_t)n_files * p->rows + 1, st));
  RPT_TRY(h->bnd.ensure((size_t)std::max<int64_t>(8, polar_bounds_words()), st));
  const size_t down_bytes = sizeof(int64_t) * (size_t)(n_files + 2) + 16;
  RPT_TRY(S.down.ensure(down_bytes, st));
  const bool grouped = polar_grouped_u8(echo, p->echo_dtype, p->bins);
  uint32_t* mk = nullptr;  // staged kept samples, as in rpt_stack_run
  if (grouped && ab().k1_stage) {
    RPT_TRY(S.k1_stage.ensure((size_t)polar_stage_words(n_files, p->rows), st));
    mk = S.k1_stage.p;
  }
  RPT_TRY(polar_count(echo, p->echo_dtype, n_files, p->rows, p->bins, p->threshold, p->stride,
                      S.row_prefix.p, S.file_off.p, nullptr, st, mk));
  int64_t spec_cap = -1;
  const int64_t* n_dev = S.file_off.p + n_files;
  // the expand write leaves the xy bounds in h->bnd itself; otherwise a bounds pass over the
  // first n_max points (n_cnt: the count on the device while the write is speculative)
  auto bounds_unless = [&](bool fused, int64_t n_max, const int64_t* n_cnt) -> int32_t {
    if (!fused) {
      hipLaunchKernelGGL(k_init_bounds, dim3(1), dim3(64), 0, st, h->bnd.p);
      hipLaunchKernelGGL(k_xy_bounds_part, dim3(grid_for(std::max<int64_t>(n_max, 1), 256, 512)),
                         dim3(256), 0, st, S.x.p, S.y.p, n_max, n_cnt, h->bnd.p);
    }
    RPT_CHECK_LAUNCH();
    return RPT_OK;
  };
  if (grouped && S.x.p && S.y.p && S.v.p && S.g.p && S.pf.p) {
    // the write and the bounds are queued with the previous run's capacity; both are redone
    // below when the count exceeds it
    spec_cap = (int64_t)std::min({S.x.cap, S.y.cap, S.v.cap, S.g.cap, S.pf.cap});
    bool fused = false;
    RPT_TRY(polar_write_cap((const uint8_t*)echo, n_files, p->rows, p->threshold, p->stride,
                            scale, cos_t, sin_t, gain, S.row_prefix.p, S.file_off.p, G, S.x.p,
                            S.y.p, S.v.p, gain ? S.g.p : nullptr, S.pf.p, spec_cap, st, mk,
                            mk ? h->bnd.p : nullptr, &fused));
    RPT_TRY(bounds_unless(fused, spec_cap, n_dev));
  }
  // one readback: file offsets (their last entry is the count) and the bounds
  int64_t* hfo = reinterpret_cast<int64_t*>(S.down.p);
  RPT_HIP(hipMemcpyAsync(hfo, S.file_off.p, sizeof(int64_t) * (n_files + 1),
                         hipMemcpyDeviceToHost, st));
  uint32_t* hb = reinterpret_cast<uint32_t*>(hfo + n_files + 1);
  if (spec_cap >= 0)
    RPT_HIP(hipMemcpyAsync(hb, h->bnd.p, 16, hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  const int64_t N = hfo[n_files];
  if (N > spec_cap) {
    const size_t cap = (size_t)std::max<int64_t>(N, 1);
    RPT_TRY(S.x.ensure(cap, st));
    RPT_TRY(S.y.ensure(cap, st));
    RPT_TRY(S.v.ensure(cap, st));
    RPT_TRY(S.g.ensure(cap, st));
    RPT_TRY(S.pf.ensure(cap, st));
    bool fused = false;
    RPT_TRY(polar_write(echo, p->echo_dtype, n_files, p->rows, p->bins, scale, cos_t, sin_t, gain,
                        p->threshold, p->stride, S.row_prefix.p, S.file_off.p, G, S.x.p, S.y.p,
                        S.v.p, gain ? S.g.p : nullptr, S.pf.p, st, mk, mk ? h->bnd.p : nullptr,
                        &fused));
    RPT_TRY(bounds_unless(fused, N, nullptr));
    RPT_HIP(hipMemcpyAsync(hb, h->bnd.p, 16, hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
  }
  const int32_t built = S.set_fo_k1(hfo, F, G);
  h->n_points = N;
  h->info = rpt_shard_info{};
  rpt_shard_info& I = h->info;
  I.n_points = N;
  I.n_built = built;
  I.halo_frames = h->hf;
  if (N > 0) {
    for (int k = 0; k < 4; ++k) I.bounds[k] = ord2f(hb[k]);
  } else {
    I.bounds[0] = I.bounds[2] = INFINITY;
    I.bounds[1] = I.bounds[3] = -INFINITY;
  }
  I.n_head_k1 = S.fo_k1[(size_t)h->hf];
  I.n_tail_k1 = N - S.fo_k1[(size_t)(F - h->hf)];
  I.n_kept = N;
  *info = I;
  return RPT_OK;
}

int64_t rpt_shard_land_cells(const float* gbounds, double resolution) {
  if (!gbounds) return 0;
  return land_edges(gbounds, resolution).cells();
}

int32_t rpt_shard_land_grid(rpt_shard* h, const float* gbounds, double* grid, int64_t cells,
                            void* stream) {
  clear_error();
  if (!h || !gbounds || !grid) {
    set_error("rpt_shard_land_grid: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  rpt_stack& S = h->st;
  const LandEdges e = land_edges(gbounds, h->p.land_resolution);
  const int32_t nxe = e.nxe(), nye = e.nye();
  if (e.cells() == 0 || e.cells() != cells) {
    set_error("rpt_shard_land_grid: grid of %lld cells does not match the bounds",
              (long long)cells);
    return RPT_EINVAL;
  }
  RPT_TRY(S.upload_land_edges(e, nullptr, 0, st, nullptr));
  const size_t cap = (size_t)std::max<int64_t>(h->n_points, 1);
  RPT_TRY(S.land_cnt.ensure((size_t)cells, st));
  RPT_TRY(S.land_cell.ensure(cap, st));
  RPT_TRY(land_grid_cells(S.x.p, S.y.p, S.v.p, h->n_points, S.edges.p, nxe, S.edges.p + nxe,
                          nye, S.land_cnt.p, grid + cells, S.land_cell.p, st,
                          h->p.echo_dtype == RPT_ECHO_U8 ? 1 : 0));
  hipLaunchKernelGGL(k_cnt_to_f64, dim3(grid_for(cells, 256, 1024)), dim3(256), 0, st,
                     S.land_cnt.p, cells, grid);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t rpt_shard_halo(rpt_shard* h, const double* grid, int64_t cells, int32_t n_built_global,
                       int32_t rank, int64_t frame0, int32_t* send_prev, int32_t* send_next,
                       int64_t recv_cap_prev, int64_t recv_cap_next, void* stream) {
  clear_error();
  if (!h || rank < 0 || recv_cap_prev < 0 || recv_cap_next < 0) {
    set_error("rpt_shard_halo: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  rpt_stack& S = h->st;
  const int32_t F = h->F;
  const int64_t N = h->n_points;
  h->rank = rank;
  h->frame0 = frame0;
  RPT_TRY(S.new_off.ensure((size_t)F + 2, st));
  RPT_TRY(S.scal.ensure(4, st));
  h->land = grid != nullptr && cells > 0;
  if (h->land) {
    RPT_TRY(S.land_cnt.ensure((size_t)cells, st));
    RPT_TRY(S.land_mask.ensure((size_t)cells, st));
    hipLaunchKernelGGL(k_f64_to_cnt, dim3(grid_for(cells, 256, 1024)), dim3(256), 0, st, grid,
                       cells, S.land_cnt.p, reinterpret_cast<int64_t*>(S.scal.p));
    RPT_CHECK_LAUNCH();
    RPT_TRY(land_mask_dev(S.land_cnt.p, grid + cells, cells, n_built_global, h->p.land_persistence,
                          h->p.land_min_intensity, S.land_mask.p,
                          reinterpret_cast<int32_t*>(S.scal.p), st));
    const size_t cap = (size_t)std::max<int64_t>(N, 1);
    RPT_TRY(S.v2.ensure(cap, st));
    RPT_TRY(S.g2.ensure(cap, st));
    RPT_TRY(S.pf2.ensure(cap, st));
    RPT_TRY(S.bnd.ensure(2 * sizeof(Bounds), st));
    // the window's arrays: [prev halo capacity | own (<= N) | next halo capacity]; the fused
    // compaction (kept points in order, new frame offsets and the own points' ST-DBSCAN bounds
    // on the device) writes x / y / t (= frame0 + frame slot) straight into the own part, so the
    // window phase only places the halo points around them
    const int64_t wcap = std::max<int64_t>(recv_cap_prev + N + recv_cap_next, 1);
    RPT_TRY(h->X.ensure((size_t)wcap, st));
    RPT_TRY(h->Y.ensure((size_t)wcap, st));
    RPT_TRY(h->T.ensure((size_t)wcap, st));
    h->direct = true;
    h->own_off = recv_cap_prev;
    h->own_cap_next = recv_cap_next;
    if (N > 0)
      RPT_TRY(land_compact_dev(S.x.p, S.y.p, S.v.p, S.had_gain ? S.g.p : nullptr, S.pf.p, N,
                               S.land_cell.p, S.land_mask.p, F, h->X.p + h->own_off,
                               h->Y.p + h->own_off, S.v2.p, S.had_gain ? S.g2.p : nullptr,
                               S.pf2.p, h->T.p + h->own_off, S.new_off.p,
                               reinterpret_cast<Bounds*>(S.bnd.p), st, frame0));
    else {
      RPT_HIP(hipMemsetAsync(S.new_off.p, 0, sizeof(int64_t) * (F + 1), st));
      hipLaunchKernelGGL(k_empty_bounds, dim3(1), dim3(64), 0, st,
                         reinterpret_cast<Bounds*>(S.bnd.p));
      RPT_CHECK_LAUNCH();
    }
  } else {
    h->direct = false;
    h->own_off = 0;
    RPT_HIP(hipMemsetAsync(S.scal.p, 0, sizeof(int64_t), st));  // (read back with the window)
    // no land filter: the kept points are the K1 points, offsets from the host copy
    RPT_TRY(S.up.ensure(sizeof(int64_t) * (size_t)(F + 1), st));
    std::memcpy(S.up.p, S.fo_k1.data(), sizeof(int64_t) * (F + 1));
    RPT_HIP(hipMemcpyAsync(S.new_off.p, S.up.p, sizeof(int64_t) * (F + 1), hipMemcpyHostToDevice,
                           st));
  }
  S.land_applied = h->land;
  if (send_prev || send_next) {
    const int64_t m = std::max(h->info.n_head_k1, h->info.n_tail_k1);
    hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(std::max<int64_t>(m, 1), 256, 1024)), dim3(256),
                       0, st, h->own_x(), h->own_y(), h->own_pf(), S.new_off.p, F, h->hf, frame0,
                       send_prev, h->info.n_head_k1, send_next, h->info.n_tail_k1);
    RPT_CHECK_LAUNCH();
  }
  return RPT_OK;
}

int32_t rpt_shard_window(rpt_shard* h, const int32_t* recv_prev, int64_t cap_prev,
                         const int32_t* recv_next, int64_t cap_next, uint8_t* flags_prev,
                         uint8_t* flags_next, rpt_shard_info* info, void* stream) {
  clear_error();
  if (!h || !info || cap_prev < 0 || cap_next < 0 || (cap_prev > 0 && !recv_prev) ||
      (cap_next > 0 && !recv_next)) {
    set_error("rpt_shard_window: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  rpt_stack& S = h->st;
  const int32_t F = h->F;
  const int64_t N = h->n_points;
  if (h->direct && (cap_prev != h->own_off || cap_next != h->own_cap_next)) {
    set_error("rpt_shard_window: halo capacities %lld / %lld differ from rpt_shard_halo's "
              "%lld / %lld", (long long)cap_prev, (long long)cap_next, (long long)h->own_off,
              (long long)h->own_cap_next);
    return RPT_EINVAL;
  }
  const int64_t wcap = std::max<int64_t>(cap_prev + N + cap_next, 1);
  if (!h->direct) {
    RPT_TRY(h->X.ensure((size_t)wcap, st));
    RPT_TRY(h->Y.ensure((size_t)wcap, st));
    RPT_TRY(h->T.ensure((size_t)wcap, st));
  }
  const size_t bb = stdbscan_bounds_bytes();
  const size_t part = stdbscan_bounds_part_bytes(wcap);
  RPT_TRY(h->wbnd.ensure(sizeof(WinMeta) + bb + part + sizeof(Bounds) + 256, st));
  WinMeta* meta = reinterpret_cast<WinMeta*>(h->wbnd.p);
  char* bnd = h->wbnd.p + sizeof(WinMeta);
  char* bpart = bnd + align_up(bb, 16);
  if (h->direct) {
    // (halo partials: at most grid_for(cap_prev + cap_next) <= grid_for(wcap), + the own one)
    const int nbh = grid_for(std::max<int64_t>(cap_prev + cap_next, 1), kBoundsBlock, 1024);
    hipLaunchKernelGGL(k_window_halo, dim3(nbh), dim3(kBoundsBlock), 0, st,
                       cap_prev > 0 ? recv_prev : nullptr, cap_prev,
                       cap_next > 0 ? recv_next : nullptr, cap_next, S.new_off.p, F, h->hf,
                       h->own_off, h->X.p, h->Y.p, h->T.p, meta,
                       reinterpret_cast<Bounds*>(bpart), nbh,
                       reinterpret_cast<const Bounds*>(S.bnd.p));
    RPT_CHECK_LAUNCH();
    RPT_TRY(stdbscan_bounds_final_dev(bpart, nbh + 1, bnd, st));
  } else {
    // (the partials' count is the bounds pass's grid: stdbscan_bounds_part_bytes)
    const int nbw = grid_for(wcap, kBoundsBlock, 1024);
    hipLaunchKernelGGL(k_window, dim3(nbw), dim3(kBoundsBlock), 0, st,
                       cap_prev > 0 ? recv_prev : nullptr, cap_prev,
                       cap_next > 0 ? recv_next : nullptr, cap_next, h->own_x(), h->own_y(),
                       h->own_pf(), S.new_off.p, F, h->hf, h->frame0, h->X.p, h->Y.p, h->T.p, meta,
                       reinterpret_cast<Bounds*>(bpart));
    RPT_CHECK_LAUNCH();
    RPT_TRY(stdbscan_bounds_final_dev(bpart, nbw, bnd, st));
  }
  // ONE readback: window counts, grid bounds, land-cell count, the kept frame offsets
  PackList pl;
  pl.add(meta, sizeof(WinMeta));
  pl.add(bnd, align_up(bb, 8));
  pl.add(S.scal.p, sizeof(int64_t));
  pl.add(S.new_off.p, sizeof(int64_t) * (F + 1));
  RPT_TRY(S.pack_d.ensure((size_t)pl.off[pl.k], st));
  RPT_TRY(S.down.ensure(sizeof(uint32_t) * (size_t)pl.off[pl.k], st));
  RPT_TRY(pack_arrays(pl, S.pack_d.p, st));
  RPT_HIP(hipMemcpyAsync(S.down.p, S.pack_d.p, sizeof(uint32_t) * (size_t)pl.off[pl.k],
                         hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  WinMeta hm;
  std::memcpy(&hm, S.down.p, sizeof(WinMeta));
  std::vector<char> hb(bb);
  std::memcpy(hb.data(), S.down.p + 4 * pl.off[1], bb);
  int64_t land_cells = 0;
  std::memcpy(&land_cells, S.down.p + 4 * pl.off[2], sizeof(int64_t));
  const int64_t* hoff = reinterpret_cast<const int64_t*>(S.down.p + 4 * pl.off[3]);
  S.fo_in.assign(hoff, hoff + F + 1);
  rpt_shard_info& I = h->info;
  I.n_kept = hm.n_own;
  I.n_head = hm.n_head;
  I.n_tail = hm.n_tail;
  I.n_prev = hm.n_prev;
  I.n_next = hm.n_next;
  I.n_land_cells = h->land ? land_cells : 0;
  h->k_prev_total = hm.k_prev_total;
  h->n_window = hm.n_window;
  S.n_frames = F;
  S.n_in = hm.n_own;
  *info = I;
  const int64_t n = hm.n_window;
  h->win_base = h->direct ? h->own_off - hm.n_prev : 0;
  if (n <= 0) return RPT_OK;
  // grid build sized on the host from the bounds just read, then K5
  const int64_t wb = h->win_base;
  RPT_TRY(dbscan_build_given(h->db, h->X.p + wb, h->Y.p + wb, h->T.p + wb, n, h->p.eps_space,
                             h->p.eps_time, h->p.min_samples, hb.data(), st));
  if (h->p.timing) {
    if (!h->ev_ok) {
      RPT_HIP(hipEventCreate(&h->ev[0]));
      RPT_HIP(hipEventCreate(&h->ev[1]));
      h->ev_ok = true;
    }
    RPT_HIP(hipEventRecord(h->ev[0], st));
  }
  RPT_TRY(dbscan_core(h->db, nullptr, st));  // (flags stay in sorted order)
  if (h->p.timing) RPT_HIP(hipEventRecord(h->ev[1], st));
  h->core_timed = h->p.timing != 0;
  // the own edge points' flags for the neighbours (their halo), straight into the send buffers
  RPT_TRY(dbscan_core_edges(h->db, hm.n_prev, hm.n_prev + hm.n_head, flags_prev,
                            hm.n_prev + hm.n_own - hm.n_tail, hm.n_prev + hm.n_own, flags_next,
                            st));
  return RPT_OK;
}

double rpt_shard_core_ms(rpt_shard* h) {
  if (!h || !h->core_timed) return -1.0;
  float ms = 0.f;
  if (hipEventSynchronize(h->ev[1]) != hipSuccess ||
      hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) != hipSuccess)
    return -1.0;
  return ms;
}

int32_t rpt_shard_link(rpt_shard* h, const uint8_t* flags_prev, const uint8_t* flags_next,
                       int64_t* comp_prev, int64_t* comp_next, void* stream) {
  clear_error();
  if (!h || (h->info.n_prev > 0 && !flags_prev) || (h->info.n_next > 0 && !flags_next)) {
    set_error("rpt_shard_link: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  const int64_t n = h->n_window;
  if (n <= 0) return RPT_OK;
  const rpt_shard_info& I = h->info;
  // halo points take their owners' flags (the owners see all their neighbours)
  RPT_TRY(h->comp.ensure((size_t)n, st));
  RPT_TRY(dbscan_set_core_edges(h->db, I.n_prev > 0 ? flags_prev : nullptr, I.n_prev,
                                I.n_next > 0 ? flags_next : nullptr, I.n_prev + I.n_kept, st));
  // component ids only where they are read: the halo points (k_pairs) and the own edge points
  // sent to the neighbours (k_comp_send); the labels take each root's representative directly
  // (k_root_reps)
  const int64_t lo_end = I.n_prev + (comp_prev ? I.n_head : 0);
  const int64_t hi_begin = I.n_prev + I.n_kept - (comp_next ? I.n_tail : 0);
  RPT_TRY(dbscan_components_edges(h->db, h->comp.p, lo_end, hi_begin, st));
  if ((comp_prev && I.n_head > 0) || (comp_next && I.n_tail > 0)) {
    hipLaunchKernelGGL(k_comp_send,
                       dim3(grid_for(std::max<int64_t>(std::max(I.n_head, I.n_tail), 1), 256, 1024)),
                       dim3(256), 0, st, h->comp.p, h->ids(), I.n_head, I.n_tail, comp_prev,
                       comp_next);
    RPT_CHECK_LAUNCH();
  }
  return RPT_OK;
}

int32_t rpt_shard_pairs(rpt_shard* h, const int64_t* owner_prev, const int64_t* owner_next,
                        int64_t* pairs, int64_t cap, void* stream) {
  clear_error();
  const rpt_shard_info& I = h ? h->info : rpt_shard_info{};
  if (!h || !pairs || cap < 0 || (I.n_prev > 0 && !owner_prev) ||
      (I.n_next > 0 && !owner_next)) {
    set_error("rpt_shard_pairs: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  RPT_TRY(h->cnt64.ensure(2, st));
  auto* cnt = reinterpret_cast<unsigned long long*>(h->cnt64.p);
  uint64_t tsize = 64;
  while (tsize < (uint64_t)(2 * (I.n_prev + I.n_next))) tsize <<= 1;
  RPT_TRY(h->pset.ensure((size_t)tsize, st));
  hipLaunchKernelGGL(k_pairs_init, dim3(grid_for((int64_t)tsize, 256, 1024)), dim3(256), 0, st,
                     cnt, h->pset.p, tsize);
  const WinIds w = h->ids();
  if (I.n_prev > 0 && h->n_window > 0)
    hipLaunchKernelGGL(k_pairs, dim3(grid_for(I.n_prev, 256, 1024)), dim3(256), 0, st, h->comp.p,
                       (int64_t)0, w, owner_prev, I.n_prev, cap, cnt, h->pset.p, tsize - 1,
                       pairs);
  if (I.n_next > 0 && h->n_window > 0)
    hipLaunchKernelGGL(k_pairs, dim3(grid_for(I.n_next, 256, 1024)), dim3(256), 0, st, h->comp.p,
                       I.n_prev + I.n_kept, w, owner_next, I.n_next, cap, cnt, h->pset.p,
                       tsize - 1, pairs);
  hipLaunchKernelGGL(k_store_count, dim3(1), dim3(64), 0, st, cnt, pairs);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t rpt_shard_finish(rpt_shard* h, const int64_t* gathered_pairs, int32_t world,
                         int64_t row_words, const int64_t* own_pairs, const int64_t* keys_host,
                         const int64_t* vals_host, int64_t n_keys, int32_t force_radix,
                         int64_t* out, int64_t out_cap, void* stream) {
  clear_error();
  if (!h || !out || out_cap < kHdr || world < 1 || (gathered_pairs && row_words < 1) ||
      (!gathered_pairs && n_keys > 0 && (!keys_host || !vals_host))) {
    set_error("rpt_shard_finish: bad arguments");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  rpt_stack& S = h->st;
  const int64_t n = h->n_window, K = h->info.n_kept;
  const int32_t F = h->F;
  if (force_radix) h->k9_radix = true;
  // ---- equivalence table (keys sorted, vals = class minimum), identical on every rank
  const int64_t keys_cap = gathered_pairs ? (int64_t)kMergeMax : std::max<int64_t>(n_keys, 1);
  RPT_TRY(h->keys.ensure((size_t)keys_cap, st));
  RPT_TRY(h->vals.ensure((size_t)keys_cap, st));
  RPT_TRY(h->meta.ensure(4, st));
  if (gathered_pairs) {
    hipLaunchKernelGGL(k_merge_pairs, dim3(1), dim3(1024), 0, st, gathered_pairs, world,
                       row_words, (int)h->merge_max, h->keys.p, h->vals.p, h->meta.p);
    RPT_CHECK_LAUNCH();
  } else {
    RPT_TRY(S.up.ensure(sizeof(int64_t) * (size_t)(2 * n_keys + 2), st));
    int64_t* hu = reinterpret_cast<int64_t*>(S.up.p);
    hu[0] = n_keys;
    hu[1] = 0;
    if (n_keys > 0) {
      std::memcpy(hu + 2, keys_host, sizeof(int64_t) * n_keys);
      std::memcpy(hu + 2 + n_keys, vals_host, sizeof(int64_t) * n_keys);
      RPT_HIP(hipMemcpyAsync(h->keys.p, hu + 2, sizeof(int64_t) * n_keys, hipMemcpyHostToDevice,
                             st));
      RPT_HIP(hipMemcpyAsync(h->vals.p, hu + 2 + n_keys, sizeof(int64_t) * n_keys,
                             hipMemcpyHostToDevice, st));
    }
    RPT_HIP(hipMemcpyAsync(h->meta.p, hu, 2 * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // the upload buffer is reused only after the next readback (a sync) of this handle
  }
  // ---- representatives: rep per window point, the sorted list of those the window sees
  const WinIds w = h->ids();
  RPT_TRY(h->rep.ensure((size_t)std::max<int64_t>(n, 1), st));
  const size_t lw = (size_t)(2 * ((keys_cap + n + 63) / 64));  // list words (k_reps)
  RPT_TRY(h->flag.ensure(std::max((size_t)(keys_cap + n + 1), 2 * lw), st));
  RPT_TRY(h->pos.ensure(std::max((size_t)(keys_cap + n + 1), lw + 1), st));
  RPT_TRY(h->reps.ensure((size_t)(keys_cap + n + 1), st));
  // list entries as bits: nw words (a multiple of two), their popcounts after them in flag
  const int64_t nw = 2 * ((keys_cap + n + 63) / 64);
  uint32_t* rbits = reinterpret_cast<uint32_t*>(h->flag.p);
  int32_t* rcnt = h->flag.p + nw;
  if (n > 0) {
    hipLaunchKernelGGL(k_reps_keys, dim3(grid_for(keys_cap + n, 256, 4096)), dim3(256), 0, st, n,
                       w, h->keys.p, h->vals.p, h->meta.p, keys_cap, rbits, rcnt);
    const uint8_t* dcore;
    const int32_t *dpar, *dsorig;
    int64_t dn = 0;
    dbscan_uf_arrays(h->db, &dcore, &dpar, &dsorig, &dn);
    hipLaunchKernelGGL(k_root_reps, dim3(grid_for(dn, 256, 4096)), dim3(256), 0, st, dcore, dpar,
                       dsorig, dn, w, h->keys.p, h->vals.p, h->meta.p, keys_cap, h->rep.p, rbits,
                       rcnt);
    RPT_CHECK_LAUNCH();
    RPT_TRY(exclusive_scan_total_i32_to_i64(rcnt, h->pos.p, nw, st));
    hipLaunchKernelGGL(k_reps_write, dim3(grid_for(keys_cap + n, 256, 4096)), dim3(256), 0, st,
                       rbits, h->pos.p, keys_cap, n, w, h->keys.p, h->reps.p);
    RPT_CHECK_LAUNCH();
  } else {
    RPT_HIP(hipMemsetAsync(h->pos.p + nw, 0, sizeof(int64_t), st));
  }
  const int64_t* nr_dev = h->pos.p + nw;
  // ---- labels of the window (local numbering), K9 of the own points
  RPT_TRY(h->labels.ensure((size_t)std::max<int64_t>(n, 1), st));
  if (n > 0) RPT_TRY(dbscan_labels_global_dev(h->db, h->rep.p, h->reps.p, nr_dev, h->labels.p, st));
  RPT_TRY(S.ensure_segs((size_t)std::max<int64_t>(K, 1), F, st));
  const int32_t* nseg_dev = nullptr;
  if (K > 0) {
    // label bits only matter on the radix path; the labels are below keys_cap + n
    const int bits = radix_bits_for(keys_cap + n);
    RPT_TRY(cluster_summaries_dev(h->labels.p + h->info.n_prev, h->own_x(), h->own_y(),
                                  h->own_v(), h->own_pf(), K, F, bits, K, S.seg_frame.p,
                                  S.seg_label.p, S.seg_count.p, S.seg_first.p, S.seg_cx.p,
                                  S.seg_cy.p, S.seg_mi.p, S.first_noise.p, &nseg_dev,
                                  h->k9_radix, nullptr, st));
  } else if (F > 0) {  // no own point: every frame without noise
    RPT_HIP(hipMemsetAsync(S.first_noise.p, 0xFF, sizeof(int64_t) * F, st));
  }
  const int64_t pair_cap = row_words > 0 ? (row_words - 1) / 2 : 0;
  hipLaunchKernelGGL(k_shard_pack, dim3(grid_for(std::max<int64_t>(K, F) + 1, 256, 512)),
                     dim3(256), 0, st, nseg_dev, nr_dev, h->meta.p, own_pairs, pair_cap,
                     S.seg_pack(), h->reps.p, S.file_off.p, h->G, F, h->frame0, K, out, out_cap);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t rpt_shard_labels(const rpt_shard* h, const int32_t* local_to_global, int64_t n_reps,
                         int32_t* out, void* stream) {
  clear_error();
  if (!h || !out || n_reps < 0 || (n_reps > 0 && !local_to_global)) {
    set_error("rpt_shard_labels: bad arguments");
    return RPT_EINVAL;
  }
  const int64_t K = h->info.n_kept;
  if (K == 0) return RPT_OK;
  if (!h->labels.p || h->labels.cap < (size_t)(h->info.n_prev + K)) {
    set_error("rpt_shard_labels: no labels (rpt_shard_finish first)");
    return RPT_EINVAL;
  }
  hipLaunchKernelGGL(k_map_labels, dim3(grid_for(K, 256, 4096)), dim3(256), 0, as_stream(stream),
                     h->labels.p + h->info.n_prev, K, local_to_global, n_reps, out);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

// (rank 0's host stage and the equivalence merge: shard_host.cpp)

int32_t rpt_shard_set_merge_limit(rpt_shard* h, int32_t max_ids) {
  clear_error();
  if (!h || max_ids < 0) {
    set_error("rpt_shard_set_merge_limit: bad arguments");
    return RPT_EINVAL;
  }
  h->merge_max = std::min<int32_t>(max_ids, kMergeMax);
  return RPT_OK;
}

int32_t rpt_shard_points(const rpt_shard* h, float* x, float* y, float* intensity,
                         int32_t* point_frame, uint8_t* core, void* stream) {
  clear_error();
  if (!h) {
    set_error("rpt_shard_points: bad arguments");
    return RPT_EINVAL;
  }
  const int64_t K = h->info.n_kept;
  if (K == 0) return RPT_OK;
  if (core && h->n_window < h->info.n_prev + K) {
    set_error("rpt_shard_points: no core flags (rpt_shard_window first)");
    return RPT_EINVAL;
  }
  const hipStream_t st = as_stream(stream);
  if (core) {  // the window's final core flags in original order (checks only)
    RPT_TRY(h->core.ensure((size_t)h->n_window, st));
    RPT_TRY(dbscan_core_orig(h->db, h->core.p, st));
  }
  auto cp = [&](void* dst, const void* src, size_t bytes) -> int32_t {
    if (dst) RPT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return RPT_OK;
  };
  RPT_TRY(cp(x, h->own_x(), sizeof(float) * (size_t)K));
  RPT_TRY(cp(y, h->own_y(), sizeof(float) * (size_t)K));
  RPT_TRY(cp(intensity, h->own_v(), sizeof(float) * (size_t)K));
  RPT_TRY(cp(point_frame, h->own_pf(), sizeof(int32_t) * (size_t)K));
  RPT_TRY(cp(core, h->core.p + h->info.n_prev, (size_t)K));
  return RPT_OK;
}

int32_t rpt_shard_frame_offsets(const rpt_shard* h, int32_t which, int64_t* out) {
  if (!h) return RPT_EINVAL;
  return rpt_stack_frame_offsets(&h->st, which, out);
}

}  // extern "C"
