// Native driver of the single-device stack path: the compute stages of run_pipeline
// (PointCloudWork/4_temporal_object_tracker.py:941-991) over a stack of sweeps already in HBM,
//
//   K1 polar scatter + fusion -> land filter (> 10 built frames, :954) -> ST-DBSCAN over the
//   stack -> per-(frame, label) summaries,
//
// in ONE library call.  The data-dependent sizes (points per file, land-filter bounds and kept
// count, grid bounds, segment count) still need host readbacks, but each is a pinned-memory copy
// and a stream sync inside C++ instead of a Python round trip per stage, and the results come
// back in one packed copy.  Buffers are owned by the handle and grow only.
#include "stack_impl.h"

namespace rpt {

// np.arange(lo, hi + res, res) for float32 lo/hi (numpy 2.x, NEP 50 weak Python floats): the
// stop and the length are float32 arithmetic, element 1 is float32(lo + res), the rest are
// float64 start + i * (e1 - e0).  Checked against numpy in tests/test_host_native.py.
std::vector<double> arange_edges(float lo, float hi, double res) {
  const float rf = (float)res;
  const float stop = hi + rf;
  const float q = (stop - lo) / rf;
  const double len_d = std::ceil((double)q);
  const int64_t len = (len_d > 0.0) ? (int64_t)len_d : 0;
  std::vector<double> e((size_t)len);
  if (len == 0) return e;
  e[0] = (double)lo;
  if (len == 1) return e;
  e[1] = (double)(float)(lo + rf);
  const double d = e[1] - e[0];
  for (int64_t i = 2; i < len; ++i) e[(size_t)i] = e[0] + (double)i * d;
  return e;
}

namespace {

__global__ void k_pack_segs(const int32_t* __restrict__ n_seg, const int32_t* __restrict__ ncl,
                            SegPack a, int64_t sc, int32_t F, char* __restrict__ out) {
  const int64_t S = *n_seg;
  const int64_t m = S < sc ? S : sc;
  const SegPackOut o(out, sc, F);
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) {
    o.hdr[0] = S;
    o.hdr[1] = ncl ? (int64_t)*ncl : -1;
  }
  for (int64_t i = i0; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    o.count[i] = a.count[i];
    o.first[i] = a.first[i];
    o.frame[i] = a.frame[i];
    o.label[i] = a.label[i];
    o.cx[i] = a.cx[i];
    o.cy[i] = a.cy[i];
    o.mi[i] = a.mi[i];
  }
  for (int64_t i = i0; i < F; i += (int64_t)gridDim.x * blockDim.x) o.noise[i] = a.noise[i];
}

}  // namespace
}  // namespace rpt

using namespace rpt;

namespace {
// One run's K1 turn at a gate (nullable: no gate, no-op).  enter() waits for the turn and makes
// the stream wait for the previous K1; leave() records this K1's end and passes the turn (also
// on an error path, from the destructor, so no later run waits forever).
class K1Turn {
 public:
  K1Turn(rpt_k1_gate* g, hipStream_t st) : g_(g), st_(st) {}
  int32_t enter() {
    if (!g_) return RPT_OK;
    std::unique_lock<std::mutex> lk(g_->mu);
    t_ = g_->issued++;
    g_->cv.wait(lk, [&] { return g_->next == t_; });
    in_ = true;
    if (t_ > 0) RPT_HIP(hipStreamWaitEvent(st_, g_->ev[(t_ - 1) % rpt_k1_gate::kRing], 0));
    return RPT_OK;
  }
  int32_t leave() {
    if (!g_ || !in_) return RPT_OK;
    in_ = false;
    std::lock_guard<std::mutex> lk(g_->mu);
    const hipError_t e = hipEventRecord(g_->ev[t_ % rpt_k1_gate::kRing], st_);
    g_->next = t_ + 1;
    g_->cv.notify_all();
    RPT_HIP(e);
    return RPT_OK;
  }
  ~K1Turn() { (void)leave(); }

 private:
  rpt_k1_gate* g_;
  hipStream_t st_;
  int64_t t_ = -1;
  bool in_ = false;
};
}  // namespace

int32_t rpt_stack::run(const rpt_stack_params& p, const void* echo, const float* scale,
                       const float* cos_t, const float* sin_t, const int32_t* gain,
                       rpt_stack_result* out, hipStream_t st) {
  const int32_t F = p.n_frames;
  if (F < 0 || p.files_per_frame < 1 || p.rows <= 0 || p.bins <= 0 || p.stride < 1 || !echo ||
      !scale || !cos_t || !sin_t) {
    set_error("rpt_stack_run: bad arguments");
    return RPT_EINVAL;
  }
  n_frames = F;
  land_applied = false;
  had_gain = gain != nullptr;
  db_state = nullptr;
  const bool timing = p.timing != 0;
  if (timing && !ev_ok) {
    for (auto& e : ev) RPT_HIP(hipEventCreate(&e));
    ev_ok = true;
  }
  if (timing) RPT_HIP(hipEventRecord(ev[0], st));
  rpt_stack_result r{};
  rpt_stack_stage s;

  RPT_TRY(run_k1(p, echo, scale, cos_t, sin_t, gain, st, s, r));
  if (timing) RPT_HIP(hipEventRecord(ev[1], st));
  fo_in = fo_k1;
  if (r.n_points == 0) {
    // no frame built: st_dbscan(frames) stacks nothing and returns {} (:463-464) -- no error,
    // no clusters, the tracker sees no frame
    RPT_TRY(wait_stream(st));
    n_in = 0;
    h_count.clear();
    h_first.clear();
    h_frame.clear();
    h_label.clear();
    h_cx.clear();
    h_cy.clear();
    h_mi.clear();
    h_noise.assign((size_t)F, -1);
    seg_hint = 0;
    if (out) *out = r;
    return RPT_OK;
  }

  RPT_TRY(run_land(p, gain, st, s, r));
  if (timing) RPT_HIP(hipEventRecord(ev[2], st));
  n_in = s.n_in;
  r.n_clustered = s.n_in;
  if (s.n_in == 0) {
    set_error("Found array with 0 sample(s) (shape=(0, 2)) while a minimum of 1 is required.");
    return RPT_EEMPTY;
  }

  RPT_TRY(run_stdbscan(p, st, s, r));
  if (timing) RPT_HIP(hipEventRecord(ev[3], st));
  RPT_TRY(run_k9(p, st, s, r));  // (records ev[4] behind its first readback copy)
  if (timing) {
    float ms[4];
    for (int k = 0; k < 4; ++k) RPT_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    r.ms_polar = ms[0];
    r.ms_land = ms[1];
    r.ms_stdbscan = ms[2];
    r.ms_summaries = ms[3];
  }
  if (out) *out = r;
  return RPT_OK;
}

int32_t rpt_stack::upload_land_edges(const LandEdges& e, const int64_t* tail, size_t n_tail,
                                     hipStream_t st, const int64_t** tail_dev) {
  const int32_t nxe = e.nxe(), nye = e.nye();
  const size_t n_up = (size_t)(nxe + nye) + n_tail;
  RPT_TRY(edges.ensure(n_up, st));
  RPT_TRY(up.ensure(sizeof(double) * n_up, st));  // its last upload completed: syncs since
  double* he = reinterpret_cast<double*>(up.p);
  std::memcpy(he, e.xe.data(), sizeof(double) * nxe);
  std::memcpy(he + nxe, e.ye.data(), sizeof(double) * nye);
  if (n_tail) std::memcpy(he + nxe + nye, tail, sizeof(int64_t) * n_tail);
  RPT_HIP(hipMemcpyAsync(edges.p, he, sizeof(double) * n_up, hipMemcpyHostToDevice, st));
  if (tail_dev) *tail_dev = reinterpret_cast<const int64_t*>(edges.p + nxe + nye);
  return RPT_OK;
}

// ---- K1: count -> per-file offsets (one readback sizes the outputs) -> write.  Leaves the
// points in x / y / v (v8) / g / pf, fo_k1, r.n_points and r.n_built, s.k1_bounds.
int32_t rpt_stack::run_k1(const rpt_stack_params& p, const void* echo, const float* scale,
                          const float* cos_t, const float* sin_t, const int32_t* gain,
                          hipStream_t st, rpt_stack_stage& s, rpt_stack_result& r) {
  const int32_t F = p.n_frames, G = p.files_per_frame;
  const int64_t n_files = (int64_t)F * G;
  RPT_TRY(file_off.ensure((size_t)n_files + 1, st));
  RPT_TRY(down.ensure(sizeof(int64_t) * (size_t)(n_files + 2 * F + 8), st));
  int64_t* hfo = reinterpret_cast<int64_t*>(down.p);
  RPT_TRY(row_prefix.ensure((size_t)n_files * p.rows + 1, st));
  // u8 sweeps of 1024 bins: the count pass stages the kept samples of every group that keeps at
  // most 128 of them (the sparse radar case) and the write pass reads those instead of the echo,
  // so K1 reads the echo once (ab().k1_stage off: two full reads)
  const bool grouped = polar_grouped_u8(echo, p.echo_dtype, p.bins);
  // the narrow point layout, on the same condition: no per-point frame slots (pf, pf2 stay
  // unallocated) -- the points are in frame order, so the land compaction, K9 and the hand-back
  // take a point's frame from the frame offsets (frame_index.h) -- and the intensities as the u8
  // samples themselves (v8, v8b instead of v, v2; float32 again on hand-back)
  narrow = grouped;
  uint32_t* mk = nullptr;
  if (grouped && ab().k1_stage) {
    RPT_TRY(k1_stage.ensure((size_t)polar_stage_words(n_files, p.rows), st));
    mk = k1_stage.p;
  }
  K1Turn k1turn(k1_gate, st);
  RPT_TRY(k1turn.enter());
  RPT_TRY(polar_count(echo, p.echo_dtype, n_files, p.rows, p.bins, p.threshold, p.stride,
                      row_prefix.p, file_off.p, nullptr, st, mk));
  RPT_HIP(hipMemcpyAsync(hfo, file_off.p, sizeof(int64_t) * (n_files + 1), hipMemcpyDeviceToHost,
                         st));
  // u8 sweeps of 1024 bins, outputs sized by an earlier run: the write is queued right behind
  // the readback (capacity-bounded) instead of after the host has seen the count; when the
  // count exceeds the capacity the buffers grow and the write runs again
  int64_t spec_cap = -1;
  // the write leaves the points' xy bounds (the land grid's edges) in k1_bnd when it takes the
  // expand path: no separate bounds pass over x and y
  if (grouped && mk) RPT_TRY(k1_bnd.ensure((size_t)polar_bounds_words(), st));
  uint32_t* kb = (grouped && mk) ? k1_bnd.p : nullptr;
  if (grouped && x.p && y.p && v8.p && g.p) {
    spec_cap = (int64_t)std::min({x.cap, y.cap, v8.cap, g.cap});
    if (!ev_rb) RPT_HIP(hipEventCreateWithFlags(&ev_rb, hipEventDisableTiming));
    RPT_HIP(hipEventRecord(ev_rb, st));
    RPT_TRY(polar_write_cap((const uint8_t*)echo, n_files, p.rows, p.threshold, p.stride, scale,
                            cos_t, sin_t, gain, row_prefix.p, file_off.p, G, x.p, y.p, v8.p,
                            gain ? g.p : nullptr, nullptr, spec_cap, st, mk, kb, &s.k1_bounds));
    RPT_HIP(hipEventSynchronize(ev_rb));  // the readback only; the write keeps running
  } else {
    RPT_TRY(wait_stream(st));
  }
  const int64_t N = hfo[n_files];
  r.n_points = N;
  r.n_built = set_fo_k1(hfo, F, G);
  const size_t cap = (size_t)std::max<int64_t>(N, 1);
  if (N > spec_cap) {
    RPT_TRY(x.ensure(cap, st));
    RPT_TRY(y.ensure(cap, st));
    RPT_TRY(g.ensure(cap, st));
    if (narrow) {
      RPT_TRY(v8.ensure(cap, st));
      RPT_TRY(polar_write((const uint8_t*)echo, n_files, p.rows, scale, cos_t, sin_t, gain,
                          p.threshold, p.stride, row_prefix.p, file_off.p, G, x.p, y.p, v8.p,
                          gain ? g.p : nullptr, nullptr, st, mk, kb, &s.k1_bounds));
    } else {
      RPT_TRY(v.ensure(cap, st));
      RPT_TRY(pf.ensure(cap, st));
      RPT_TRY(polar_write(echo, p.echo_dtype, n_files, p.rows, p.bins, scale, cos_t, sin_t, gain,
                          p.threshold, p.stride, row_prefix.p, file_off.p, G, x.p, y.p, v.p,
                          gain ? g.p : nullptr, pf.p, st, mk, kb, &s.k1_bounds));
    }
  }
  RPT_TRY(k1turn.leave());
  s.cx = x.p;
  s.cy = y.p;
  s.cv = narrow ? nullptr : v.p;
  s.cv8 = narrow ? v8.p : nullptr;
  s.cpf = narrow ? nullptr : pf.p;
  s.n_in = N;
  return RPT_OK;
}

// ---- land filter (global grid over the stack, :954 gate: more than 10 built frames).  When it
// applies, s names the kept points (x2 / y2 / ...), fo_in their frame offsets, and the kept
// points' times (t) and ST-DBSCAN bounds (dbscan_bounds) are ready.
int32_t rpt_stack::run_land(const rpt_stack_params& p, const int32_t* gain, hipStream_t st,
                            rpt_stack_stage& s, rpt_stack_result& r) {
  const int32_t F = p.n_frames;
  const int64_t N = r.n_points;
  r.n_land_cells = 0;
  if (!(p.land_filter && r.n_built > 10 && N > 0)) return RPT_OK;
  const size_t cap = (size_t)std::max<int64_t>(N, 1);
  float b4[4];
  if (s.k1_bounds) {
    uint32_t hb[4];
    RPT_HIP(hipMemcpyAsync(hb, k1_bnd.p, sizeof hb, hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
    for (int k = 0; k < 4; ++k) b4[k] = ord2f(hb[k]);
  } else {
    RPT_TRY(bounds_xy(x.p, y.p, N, b4, st));  // synchronises
  }
  // edges and the K1 frame offsets in ONE upload: [x edges | y edges | offsets (int64)]
  const LandEdges e = land_edges(b4, p.land_resolution);
  const int32_t nxe = e.nxe(), nye = e.nye();
  const int64_t cells = e.cells();
  if (cells == 0) {
    set_error("rpt_stack_run: degenerate land grid");
    return RPT_EINVAL;
  }
  const int64_t* fo_dev = nullptr;
  RPT_TRY(upload_land_edges(e, fo_k1.data(), (size_t)F + 1, st, &fo_dev));
  RPT_TRY(land_cnt.ensure((size_t)cells, st));
  RPT_TRY(land_tot.ensure((size_t)cells, st));
  RPT_TRY(land_mask.ensure((size_t)cells, st));
  // narrow path: 16-bit cell ids when the grid has at most 65,536 cells (with ab().land_u8
  // off the filter keeps its float, int32-cell form)
  const bool cell16 = narrow && cells <= 65536 && ab().land_u8;
  if (cell16)
    RPT_TRY(land_cell16.ensure(cap, st));
  else
    RPT_TRY(land_cell.ensure(cap, st));
  // the land-cell count accumulates (int32) into the low half of an int64 slot, zeroed with
  // the grid
  RPT_TRY(scal.ensure(4, st));
  RPT_TRY(land_grid_cells(x.p, y.p, s.cv, N, edges.p, nxe, edges.p + nxe, nye, land_cnt.p,
                          land_tot.p, cell16 ? nullptr : land_cell.p, st,
                          p.echo_dtype == RPT_ECHO_U8 ? 1 : 0, reinterpret_cast<int64_t*>(scal.p),
                          cell16 ? land_cell16.p : nullptr, s.cv8));
  RPT_TRY(land_mask_dev(land_cnt.p, land_tot.p, cells, r.n_built, p.land_persistence,
                        p.land_min_intensity, land_mask.p, reinterpret_cast<int32_t*>(scal.p),
                        st));
  RPT_TRY(x2.ensure(cap, st));
  RPT_TRY(y2.ensure(cap, st));
  if (narrow)
    RPT_TRY(v8b.ensure(cap, st));
  else
    RPT_TRY(v2.ensure(cap, st));
  RPT_TRY(g2.ensure(cap, st));
  if (!narrow) RPT_TRY(pf2.ensure(cap, st));
  RPT_TRY(new_off.ensure((size_t)F + 1, st));
  // one fused compaction: the kept points in order, their frame times and their ST-DBSCAN
  // bounds (the kept count new_off[F] stays on the device), read back with the offsets and the
  // land-cell count: ONE round trip
  RPT_TRY(t.ensure(cap, st));
  const size_t bnd_bytes = stdbscan_bounds_bytes();
  RPT_TRY(bnd.ensure(2 * bnd_bytes, st));
  RPT_TRY(land_compact_dev(x.p, y.p, s.cv, gain ? g.p : nullptr, s.cpf, N, land_cell.p,
                           land_mask.p, F, x2.p, y2.p, narrow ? nullptr : v2.p,
                           gain ? g2.p : nullptr, narrow ? nullptr : pf2.p, t.p, new_off.p,
                           reinterpret_cast<Bounds*>(bnd.p), st, 0, narrow ? fo_dev : nullptr,
                           cell16 ? land_cell16.p : nullptr, s.cv8, narrow ? v8b.p : nullptr));
  int64_t* hn = reinterpret_cast<int64_t*>(down.p);
  PackList pl;
  pl.add(new_off.p, sizeof(int64_t) * (F + 1));
  pl.add(scal.p, sizeof(int64_t));
  pl.add(bnd.p, bnd_bytes);
  RPT_TRY(pack_d.ensure((size_t)pl.off[pl.k], st));
  RPT_TRY(pack_arrays(pl, pack_d.p, st));
  RPT_HIP(hipMemcpyAsync(hn, pack_d.p, sizeof(uint32_t) * (size_t)pl.off[pl.k],
                         hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  fo_in.assign(hn, hn + F + 1);
  r.n_land_cells = hn[F + 1];
  dbscan_bounds.assign(reinterpret_cast<const char*>(hn + F + 2),
                       reinterpret_cast<const char*>(hn + F + 2) + bnd_bytes);
  s.cx = x2.p;
  s.cy = y2.p;
  s.cv = narrow ? nullptr : v2.p;
  s.cv8 = narrow ? v8b.p : nullptr;
  s.cpf = narrow ? nullptr : pf2.p;
  s.n_in = hn[F];
  land_applied = true;
  return RPT_OK;
}

// ---- ST-DBSCAN over the stack (times = frame slot as float32, :460-467).  Leaves labels, the
// cluster count on the device (s.ncl_dev), db_state and s.fo_k9.
int32_t rpt_stack::run_stdbscan(const rpt_stack_params& p, hipStream_t st, rpt_stack_stage& s,
                                rpt_stack_result& r) {
  const int32_t F = p.n_frames;
  RPT_TRY(labels.ensure((size_t)s.n_in, st));
  if (!land_applied) {  // with the land filter, the times and bounds came with its readback
    RPT_TRY(t.ensure((size_t)s.n_in, st));
    if (narrow) {
      // no land filter: the K1 offsets go up here (with it they rode behind the land edges)
      RPT_TRY(fo_d.ensure((size_t)F + 1, st));
      RPT_TRY(up.ensure(sizeof(int64_t) * ((size_t)F + 1), st));
      std::memcpy(up.p, fo_k1.data(), sizeof(int64_t) * ((size_t)F + 1));
      RPT_HIP(hipMemcpyAsync(fo_d.p, up.p, sizeof(int64_t) * ((size_t)F + 1),
                             hipMemcpyHostToDevice, st));
      RPT_TRY(frame_fill(fo_d.p, F, t.p, nullptr, st));
    } else {
      RPT_TRY(frame_times(s.cpf, s.n_in, nullptr, t.p, st));
    }
  }
  // the frame offsets of the points that ST-DBSCAN and K9 see, on the device (narrow path)
  s.fo_k9 = !narrow ? nullptr : land_applied ? new_off.p : fo_d.p;
  // ST-DBSCAN and K9 without readbacks in between: the cluster count and the segment count stay
  // on the device and come back with the results in ONE readback; the K9 sort runs with the
  // previous run's label bits and the summarize grid with its segment count, and both are
  // redone (rare) when the counts show they did not fit
  r.dbscan = rpt_stdbscan_stats{};
  r.dbscan.timing = p.timing;
  void* dstate = nullptr;
  RPT_TRY(stdbscan_deferred(s.cx, s.cy, nullptr, 1, t.p, s.n_in, p.eps_space, p.eps_time,
                            p.min_samples, labels.p, &r.dbscan, st, 2, &s.ncl_dev, &dstate,
                            land_applied ? dbscan_bounds.data() : nullptr));
  db_state = dstate;
  db_stream = st;
  return RPT_OK;
}

// The packed readback at capacity sc (SegPackOut): pack, copy (mark, if any, recorded behind
// it), wait; *S = the segment count the device saw (more than sc: read again at that capacity).
int32_t rpt_stack::read_segs(const int32_t* nseg_dev, const int32_t* ncl_dev, int64_t sc,
                             hipEvent_t mark, hipStream_t st, int64_t* S) {
  const int32_t F = n_frames;
  const size_t bytes = seg_pack_bytes(sc, F);
  RPT_TRY(pack_d.ensure(bytes / 4 + 1, st));
  RPT_TRY(down.ensure(bytes, st));
  hipLaunchKernelGGL(k_pack_segs, dim3(grid_for(std::max<int64_t>(sc, F), 256, 256)), dim3(256),
                     0, st, nseg_dev, ncl_dev, seg_pack(), sc, F,
                     reinterpret_cast<char*>(pack_d.p));
  RPT_CHECK_LAUNCH();
  RPT_HIP(hipMemcpyAsync(down.p, pack_d.p, bytes, hipMemcpyDeviceToHost, st));
  if (mark) RPT_HIP(hipEventRecord(mark, st));
  RPT_TRY(wait_stream(st));
  *S = SegPackOut(down.p, sc, F).hdr[0];
  return RPT_OK;
}

// ---- K9 summaries (per-(frame, label) segments), the packed readback and its redo.  Leaves the
// segments in h_*, the counts in r and next run's guesses (sum_bits, seg_hint, k9_radix).
int32_t rpt_stack::run_k9(const rpt_stack_params& p, hipStream_t st, const rpt_stack_stage& s,
                          rpt_stack_result& r) {
  const int32_t F = p.n_frames;
  RPT_TRY(ensure_segs((size_t)s.n_in, F, st));
  const int bits = s.ncl_dev ? sum_bits : radix_bits_for(r.dbscan.n_clusters);
  const int64_t sc = std::min<int64_t>(
      std::max<int64_t>(seg_hint > 0 ? seg_hint + seg_hint / 4 + 64 : 4096, 1), s.n_in);
  const int32_t* nseg_dev = nullptr;
  bool radix_used = false;
  auto k9 = [&](int bits_, int64_t sc_, bool* used) {
    return cluster_summaries_dev(labels.p, s.cx, s.cy, s.cv, s.cpf, s.n_in, F, bits_, sc_,
                                 seg_frame.p, seg_label.p, seg_count.p, seg_first.p, seg_cx.p,
                                 seg_cy.p, seg_mi.p, first_noise.p, &nseg_dev, k9_radix, used, st,
                                 s.fo_k9, s.cv8);
  };
  RPT_TRY(k9(bits, sc, &radix_used));
  int64_t S;
  RPT_TRY(read_segs(nseg_dev, s.ncl_dev, sc, p.timing ? ev[4] : nullptr, st, &S));
  const int64_t ncl = s.ncl_dev ? SegPackOut(down.p, sc, F).hdr[1] : r.dbscan.n_clusters;
  if (s.ncl_dev) RPT_TRY(stdbscan_fill_stats(db_state, (int32_t)ncl, &r.dbscan));
  int64_t sc_used = sc;
  // K9 again when the frame sort met a frame with too many labels (S = -1: the radix path, from
  // now on) or the radix path's label keys needed more bits; then the readback repeats until it
  // holds every segment (a redo changes the count)
  const bool bits_short = radix_used && (int64_t(1) << bits) <= ncl;
  if (S < 0 || bits_short || S > sc) {
    const bool rerun = S < 0 || bits_short;
    if (S < 0) k9_radix = true;
    if (rerun) RPT_TRY(k9(radix_bits_for(ncl), std::max<int64_t>(S, sc), nullptr));
    sc_used = rerun ? sc : std::max<int64_t>(S, 1);
    for (int pass = 0; pass < 2; ++pass) {
      RPT_TRY(read_segs(nseg_dev, s.ncl_dev, sc_used, nullptr, st, &S));
      if (S <= sc_used) break;
      sc_used = S;
    }
  }
  // next run's guesses: one pass of up to 12 bits when the count allows, with headroom
  const int exact = radix_bits_for(ncl);
  sum_bits = std::max(exact, std::min(radix_bits_for(2 * ncl + 64), std::max(exact, 12)));
  seg_hint = S;
  r.n_clusters = (int32_t)ncl;
  r.n_segments = S;
  const SegPackOut h(down.p, sc_used, F);
  h_count.assign(h.count, h.count + S);
  h_first.assign(h.first, h.first + S);
  h_noise.assign(h.noise, h.noise + F);
  h_frame.assign(h.frame, h.frame + S);
  h_label.assign(h.label, h.label + S);
  h_cx.assign(h.cx, h.cx + S);
  h_cy.assign(h.cy, h.cy + S);
  h_mi.assign(h.mi, h.mi + S);
  return RPT_OK;
}

extern "C" {

int32_t rpt_arange_edges(float lo, float hi, double res, double* out, int32_t cap) {
  const std::vector<double> e = arange_edges(lo, hi, res);
  if (out) std::copy(e.begin(), e.begin() + std::min<size_t>(e.size(), (size_t)std::max(cap, 0)), out);
  return (int32_t)e.size();
}

rpt_stack* rpt_stack_create(void) { return new rpt_stack(); }

rpt_k1_gate* rpt_k1_gate_create(void) {
  clear_error();
  rpt_k1_gate* g = new rpt_k1_gate();
  for (auto& e : g->ev) {
    const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (err != hipSuccess) {
      e = nullptr;
      set_error("rpt_k1_gate_create: hipEventCreateWithFlags failed: %s",
                hipGetErrorString(err));
      delete g;  // (destroys the events made so far)
      return nullptr;
    }
  }
  return g;
}

void rpt_k1_gate_destroy(rpt_k1_gate* g) { delete g; }

int32_t rpt_stack_set_k1_gate(rpt_stack* h, rpt_k1_gate* g) {
  if (!h) return RPT_EINVAL;
  h->k1_gate = g;
  return RPT_OK;
}

void rpt_stack_destroy(rpt_stack* h) { delete h; }

int32_t rpt_stack_run(rpt_stack* h, const rpt_stack_params* p, const void* echo,
                      const float* scale, const float* cos_t, const float* sin_t,
                      const int32_t* gain, rpt_stack_result* out, void* stream) {
  clear_error();
  if (!h || !p) {
    set_error("rpt_stack_run: null handle or params");
    return RPT_EINVAL;
  }
  // the run's counters from one clear of the stream's zero pool (common.h)
  RPT_TRY(zero_pool_arm(as_stream(stream)));
  return h->run(*p, echo, scale, cos_t, sin_t, gain, out, as_stream(stream));
}

int32_t rpt_stack_frame_offsets(const rpt_stack* h, int32_t which, int64_t* out) {
  if (!h || !out || (which != 0 && which != 1)) return RPT_EINVAL;
  const auto& v = which == 0 ? h->fo_k1 : h->fo_in;
  std::copy(v.begin(), v.end(), out);
  return RPT_OK;
}

int32_t rpt_stack_segments(const rpt_stack* h, int32_t* frame, int32_t* label, int64_t* count,
                           int64_t* first, float* cx, float* cy, float* mean_i,
                           int64_t* frame_first_noise) {
  if (!h) return RPT_EINVAL;
  auto cp = [](const auto& v, auto* dst) {
    if (dst) std::copy(v.begin(), v.end(), dst);
  };
  cp(h->h_frame, frame);
  cp(h->h_label, label);
  cp(h->h_count, count);
  cp(h->h_first, first);
  cp(h->h_cx, cx);
  cp(h->h_cy, cy);
  cp(h->h_mi, mean_i);
  cp(h->h_noise, frame_first_noise);
  return RPT_OK;
}

int32_t rpt_stack_points(const rpt_stack* h, float* x, float* y, float* intensity,
                         int32_t* gain, int32_t* point_frame, int32_t* labels, void* stream) {
  clear_error();
  if (!h) return RPT_EINVAL;
  const hipStream_t st = as_stream(stream);
  const size_t n = (size_t)h->n_in;
  auto cp = [&](void* dst, const void* src, size_t es) -> int32_t {
    if (dst && src && n) RPT_HIP(hipMemcpyAsync(dst, src, n * es, hipMemcpyDeviceToDevice, st));
    return RPT_OK;
  };
  if (gain && !h->had_gain) {
    set_error("rpt_stack_points: the last rpt_stack_run had no gain table, so no per-point gains");
    return RPT_EINVAL;
  }
  const bool l = h->land_applied;
  RPT_TRY(cp(x, l ? h->x2.p : h->x.p, 4));
  RPT_TRY(cp(y, l ? h->y2.p : h->y.p, 4));
  if (h->narrow) {  // kept as u8 samples: float32 again on hand-back
    if (intensity) RPT_TRY(bytes_to_float(l ? h->v8b.p : h->v8.p, (int64_t)n, intensity, st));
  } else {
    RPT_TRY(cp(intensity, l ? h->v2.p : h->v.p, 4));
  }
  RPT_TRY(cp(gain, l ? h->g2.p : h->g.p, 4));
  if (h->narrow) {  // no frame slots were kept: filled from the offsets of the handed-back points
    if (point_frame && n)
      RPT_TRY(frame_fill(l ? h->new_off.p : h->fo_d.p, h->n_frames, nullptr, point_frame, st));
  } else {
    RPT_TRY(cp(point_frame, l ? h->pf2.p : h->pf.p, 4));
  }
  RPT_TRY(cp(labels, h->labels.p, 4));
  return RPT_OK;
}

int32_t rpt_stack_core_flags(const rpt_stack* h, uint8_t* core, void* stream) {
  clear_error();
  if (!h || !core) return RPT_EINVAL;
  if (!h->db_state || h->n_in <= 0) {
    set_error("rpt_stack_core_flags: the last rpt_stack_run clustered no points");
    return RPT_EINVAL;
  }
  if (as_stream(stream) != h->db_stream) {
    set_error("rpt_stack_core_flags: call on the stream of the last rpt_stack_run");
    return RPT_EINVAL;
  }
  return stdbscan_core_flags(h->db_state, h->n_in, core, as_stream(stream));
}

}  // extern "C"

