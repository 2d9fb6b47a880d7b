// ST-DBSCAN on gfx950: uniform space x time grid, exact neighbour predicate, deterministic
// union-find labelling.  Replaces the BallTree + Python BFS of
//   PointCloudWork/3_stdbscan_point_clouds.py:101-136,
//   radar_pipeline/processors/clustering.py:49-115 and
//   PointCloudWork/4_temporal_object_tracker.py:466-506.
//
// Semantics reproduced bit-exactly:
//   nbr(i,j)  <=>  d2(i,j) <= eps^2  (float64: ((xi-xj)^2 + (yi-yj)^2 [+ (zi-zj)^2]), each op
//                  rounded, no FMA — sklearn's euclidean rdist on float64 copies of the f32 input)
//             and  |t_j - t_i| <= eps_t  (float32 arithmetic; eps_t rounded to float32 — the
//                  reference compares np.float32 values with a Python float under NEP 50)
//   core(i)   <=>  |{ j : nbr(i,j) }| >= min_samples   (the count includes i itself)
//   clusters  =    connected components of the core-core graph, numbered in ascending order of
//                  each component's minimum core-point index (the order the BFS starts them)
//   border    =    non-core point with a core neighbour: minimum adjacent cluster id
//   noise     =    -1
//
// Pipeline (K4..K8 of SURVEY.md §8a).  This file is the one translation unit: the DbscanState
// driver, the fused entry points and the phased C-ABI bodies.  Every kernel and device helper is
// in a stage file, included (inside namespace rpt { namespace {) in this order; a stage file
// reads stdbscan_shared.inc and, where its header says so, an earlier stage file, never a later
// one.  Each file's header names the state arrays its kernels read and leave behind.
//   stdbscan_shared.inc  what more than one stage or the driver reads (no kernel)
//   stdbscan_grid.inc    K4, the grid build            DbscanState::build_t
//   stdbscan_core.inc    K5, the core flags            DbscanState::core_pass
//   stdbscan_count.inc   the exact neighbour counts    DbscanState::count_pass, core_from_counts
//   stdbscan_union.inc   K6, the core-core union-find  DbscanState::union_pass
//   stdbscan_label.inc   K7/K8, ids and labels         DbscanState::cluster_ids, labels_local,
//                                                      labels_global and the phased bodies
//   stdbscan_frames.inc  the denoise variant           DbscanState::frames_pass, labels_fifo
//   stdbscan_ab.inc      the replaced forms, A/B build only (RPT_AB; included by the label file)
//
// Cell side is 0.7 eps in 2-D and eps/2 in 3-D (x (1+2^-20)): at least eps/2, so every neighbour
// lies within +-2 cells, and small enough that a full cell's diagonal (0.99 eps in 2-D,
// eps*sqrt(3)/2 in 3-D) stays within eps, so dense cells can be "mutual" (decided from their
// actual boxes, k_cell_box).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "dispatch.h"  // with_bool, with_dim
#include "stdbscan.h"

#pragma clang fp contract(off)

namespace rpt {

namespace {

#include "stdbscan_shared.inc"
#include "stdbscan_grid.inc"
#include "stdbscan_core.inc"
#include "stdbscan_count.inc"
#include "stdbscan_union.inc"
#include "stdbscan_label.inc"
#include "stdbscan_frames.inc"

struct Timer {
  bool on = false;
  hipStream_t st{};
  hipEvent_t ev[8]{};
  int k = 0;
  void start(bool enable, hipStream_t s) {
    on = enable;
    st = s;
    k = 0;
    if (!on) return;
    for (auto& e : ev)
      if (!e) (void)hipEventCreate(&e);
    (void)hipEventRecord(ev[k++], st);
  }
  void mark() {
    if (on && k < 8) (void)hipEventRecord(ev[k++], st);
  }
  double ms(int i) {
    float t = 0;
    (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
    return t;
  }
  ~Timer() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

// One ST-DBSCAN problem on one device, split in phases so that a frame-sharded multi-GPU run
// can exchange halo core flags and component ids between them.  Owns its device memory.
struct DbscanState {
  Scratch arena;
  int dim = 2;
  int64_t n = 0;
  bool degenerate = false;  // negative/NaN eps: no pair passes, not even (i, i)
  int32_t min_samples = 0;
  Geom g{};
  int64_t C = 0, nt = 0;
  float4* pts = nullptr;
  int32_t *sorig = nullptr, *skey = nullptr, *cell_start = nullptr, *rep = nullptr;
  uint8_t *mutual = nullptr, *core = nullptr;
  float2* slab_t = nullptr;
  int32_t *parent = nullptr, *ccmin = nullptr, *cid = nullptr, *nc_list = nullptr;
  int32_t *occ = nullptr, *hpos = nullptr;  // occupied cells (ascending), head-flag scan
  const int32_t* n_occ_dev = nullptr;        // the occupied-cell count (hpos[n] or the slab scan's)
  uint64_t* cell_min_pair = nullptr;         // per cell (min core original index, its sorted index)
  bool cmin_ready = false;  // cell_min_pair filled by the core pass for the current core flags
  void* crec = nullptr;                      // CellRec<dim>[C + 1]
  uint32_t* occ_bits = nullptr;              // 1 bit per cell
  // per-cell path (cell_comp): 1 bit per cell with a core point (rep[c] >= 0), every word written
  // by k_parent_init_cells, and its dilation over the label pass's window reach (integral times;
  // k_near_bits, every word written per run).  Laid out and padded as occ_bits.
  uint32_t *core_bits = nullptr, *near_bits = nullptr;
  uint4* pmask = nullptr;  // union passes' undecided-candidate masks per occupied cell (aliases
                           // the grid build's radix key buffers, dead after the build)
  // occupied cells per wave iteration of k_union_cells_pair: 64 on large stacks (one header load
  // per lane), 16 on small ones (ab().union_cpw overrides)
  int union_cpw() const {
    if (ab().union_cpw) return ab().union_cpw;
    return n > (int64_t(1) << 24) ? 64 : 16;
  }
  uint32_t* min_bits = nullptr;  // component minima, 1 bit per original index (MinRank)
  int32_t* min_pref = nullptr;   // exclusive popcount prefix of min_bits' words (+ total)
  int64_t min_words() const { return n / 32 + 1; }
  int32_t* n_clusters_ptr() const { return min_pref + min_words(); }
  int32_t cluster_ids(hipStream_t st, int32_t* cell_key, int32_t* zero = nullptr);
  int32_t* cell_root = nullptr;  // per cell: root of a mutual cell's core points (k_cell_roots)
  bool bucket_allmin = false;  // this build's cell minima came from k_slab_bucket
  // the default K5 pipeline: the cell pass writes the point flags and the queue itself, with the
  // all-core cells' minima from k_cell_box (decided at build time, before k_cell_box runs).
  // k5_mode 0 (the round-1 queue pipeline) is the default: the folded variants measured no faster
  // on the 100- and 1000-frame stacks (profiles/r2/ab_k5_k1.md): the per-point flag writes moved
  // into the cell kernel by 8 lanes per cell cost what the fill pass cost, and the cell-wise slow
  // pass balances worse than the point queue
  bool k5_fused_path() const {
    return oct_ok() && ab().k5_mode == 0 && ab().k5_fused && !ab().k5_tiles;
  }
  int32_t* rowq = nullptr;    // first occupied-list index of every (slab, row) + total (tiles)
  int32_t* rowcnt = nullptr;  // occupied cells per (slab, row)
  bool rowq_ok = false;       // rowq built for this grid (the core pass's tile path)
  int tile_by = 0, tile_nbands = 0, tile_R = 0;
  // the label pass on the core pass's tiles (rowq built, ab().k7_tiles on)
  bool use_label_tiles() const { return ab().k7_tiles && rowq_ok && dim == 2 && g.nz == 1; }
  unsigned tile_grid_blocks() const {  // the tiles + the isolated cell's, a multiple of 8
    return (unsigned)((((int64_t)g.nt * tile_nbands + 1) + 7) & ~(int64_t)7);
  }
  // slabs each side a cell's points can reach: eps_t / slab width, +1 for the slab's extent;
  // integral times with integral slab widths: a slab holds whole time values, so ceil(floor(eps_t)
  // / width) slabs each side hold every time within eps_t
  double slab_reach() const {
    return integral_t ? std::ceil(std::floor((double)g.epst) / g.ct)
                      : std::ceil((double)g.epst / g.ct) + 1.0;
  }
  // the eight-lanes-per-cell K5 / K6 kernels (2-D, at most kCwMaxR slabs each side)
  bool oct_ok() const { return dim == 2 && g.nz == 1 && slab_reach() <= (double)kCwMaxR; }
  template <int D>
  const CellRec<D>* rec() const {
    return static_cast<const CellRec<D>*>(crec);
  }
  // per original point: its sorted position (the grid build's inverse permutation, read by the
  // label passes, when spos_on); the global path then reuses it for the sorted points' final
  // core labels
  int32_t* slab = nullptr;
  bool spos_on = false;
  bool dense_slabs = false;  // more than 8 kChunkPts points per slab on average (bucket path)
  int32_t* cell_min = nullptr;  // per cell: smallest component key (label pass)
  uint8_t* fok = nullptr;    // per cell: frame condition met by every core point (denoise)
  bool integral_t = false;   // every finite t integral (slab = one frame id)
  // every occupied cell is mutual by construction: 2-D, one time value per slab (integral times,
  // ct = 1), every time finite (no isolated cell), the cell diagonal within eps (the cell side
  // not coarsened by the cell cap), min_samples >= 1.  Set by build_t.
  bool all_mutual = false;
  // this run takes the per-cell union init / component ids / core labels (all_mutual grid, the
  // fused local path with a readback of the cluster count; set by union_pass, read by
  // labels_local)
  bool cell_comp = false;
  // a fused local run on this grid takes the per-cell path (cell_comp; see union_pass)
  bool cell_comp_ok() const {
    const AbSwitches& a = ab();
    return all_mutual && dim == 2 && a.union_list && a.union_pair && a.union_nm && a.cell_comp &&
           !use_label_tiles() && !a.uf_compress;
  }
  // ... and its label stage takes k_label's candidates from core_bits: every k_label form a
  // cell_comp run can launch (32 or 64 lanes, float4 or xy points) then reads cell_min only where
  // core_bits is set, as k_label_core_cells does for core points (the label tiles rule cell_comp
  // out).  Needs the exact slab windows of integral times (an infinite eps_time has g.rt = -1).
  bool core_bits_ok() const { return cell_comp_ok() && g.rt >= 0; }
  // ... and near_bits is built and tested per non-core point in k_label_core_cells, and cell_min
  // gets no INT_MAX fill (no reader looks at a cell without core points then, see above).  Not on
  // dense slabs, where nearly every point is core and the queue is a few thousand points
  // (configs[4] share: k_label 4.8 us, against +10.7 us for k_near_bits and +23.6 us in
  // k_label_core_cells<true>); there the label stage keeps the fill as well, so its kernels run
  // as before.
  bool near_bits_ok() const { return core_bits_ok() && !dense_slabs; }
  // The sorted points are float2 {x, y} in the first half of pts' allocation (Pt<true>), not
  // float4: the build's writer was k_slab_bucket<true> / k_slab_chunk_scatter<true>.  A kernel
  // that assumed the other layout would read out of bounds, so the one rule is xy_rule() and
  // every pass that reads points through a float4 kernel refuses such a state (need_float4).
  bool xy_points = false;
  // set by the fused local drivers right before build(), consumed by it: the caller reads the
  // points only through core_pass / union_pass(fused) / labels_local
  bool may_xy = false;
  // Does every point-reading kernel the fused local run will launch on this grid know the xy
  // layout?  Those are k_cell_box / k_cell_box_mixed, k_core_slow_masked, k_union_listed and
  // k_label<2, false, 32, true> (k_union_cells_pair reads no point; the per-cell path launches
  // neither k_union_nm nor a compression pass).  Anything else turns the layout off: the other
  // K5 pipelines (RPT_K5_MODE / _TILES / _FUSED / _MASK, eps_t >= 3), the per-point union paths
  // (RPT_UNION_PAIR / _LIST / _NM, RPT_CELL_COMP=0, RPT_UF_COMPRESS=1), the label tiles and the
  // 64-lane label pass (RPT_K7_TILES, RPT_K7_W=64).  RPT_XY_POINTS=0 keeps float4 (A/B).
  bool xy_rule() const {
    const AbSwitches& a = ab();
    // (a fractional eps_t also keeps float4: its windows are tfree all the same, it is only
    // not among the cases the layout was measured and tested on)
    return a.xy_points && dim == 2 && g.tfree && g.epst == std::floor(g.epst) && cell_comp_ok() &&
           k5_fused_path() && (int)slab_reach() <= 2 && a.k5_mask && !a.k7_tiles && a.k7_w == 32;
  }
  int32_t need_float4(const char* who) const {
    if (!xy_points) return RPT_OK;
    set_error("%s: internal: this state's sorted points are xy-only", who);
    return RPT_EHIP;
  }
  // the sorted points as the kernels of one layout read or write them (XY only where
  // xy_points: the allocation's first half)
  template <bool XY>
  Pt<XY>* points() const {
    return reinterpret_cast<Pt<XY>*>(pts);
  }
  int64_t* stmp = nullptr;
  int32_t* counts = nullptr;  // count_pass's result per sorted point, for the sweep
  int32_t* n_core_dev = nullptr;
  Timer tm;

  template <int D>
  int32_t build_t(const float* x, const float* y, const float* z, int64_t stride, const float* t,
                  double eps_space, double eps_time, hipStream_t st);
  const void* given_bounds = nullptr;  // host Bounds computed by the caller (stdbscan_bounds_dev)
  int32_t build(const float* x, const float* y, const float* z, int64_t stride, const float* t,
                int64_t n_, double eps_space, double eps_time, int32_t ms, bool timing,
                hipStream_t st);
  int32_t core_pass(hipStream_t st);
  // the exact neighbour counts of the sorted points (stdbscan_count.inc), after build: no early
  // exit, no min_samples.  counts_sorted: n int32 (DbscanState::counts for the sweep)
  int32_t count_pass(int32_t* counts_sorted, hipStream_t st);
  // core[s] = counts_sorted[s] >= m (m >= 1) as the flags of the passes that follow; the number of
  // core points is left on the device at n_core_dev (a pre-zeroed pool word, common.h)
  int32_t core_from_counts(const int32_t* counts_sorted, int32_t m, hipStream_t st);
  // fused: called by the fused local path (labels_local follows, the count is read back)
  int32_t union_pass(hipStream_t st, bool fused = false);
  int32_t labels_local(int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st);
  // deferred mode: labels_local leaves the cluster count on the device (cid[n]) and the timing
  // events unread; fill_stats completes the stats once the caller has synchronised the stream
  bool defer = false;
  int32_t fill_stats(int32_t n_clusters, rpt_stdbscan_stats* stats);
  int32_t labels_global(const int64_t* rep_orig, const int64_t* reps, int64_t nr,
                        int32_t* labels, hipStream_t st, const int64_t* nr_dev = nullptr);
  // denoise variant: the min_frames core condition, then the FIFO border labels
  int32_t frames_pass(int32_t min_frames, hipStream_t st);
  int32_t labels_fifo(int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st);
};

template <int D>
int32_t DbscanState::build_t(const float* x, const float* y, const float* z, int64_t stride,
                             const float* t, double eps_space, double eps_time, hipStream_t st) {
  const int gb = grid_for(n, kBlock, 2048);
  // ---- bounds (one small sync); the arena is re-reserved below, so copy results out first
  const int nbb = grid_for(n, kBlock, 1024);
  {
    Budget bb;
    bb.add<Bounds>(1);
    bb.add<Bounds>(nbb);
    RPT_TRY(arena.reserve(bb.bytes, st));
  }
  Bounds* d_b = arena.carve_n<Bounds>(1);
  Bounds* d_part = arena.carve_n<Bounds>(nbb);
  Bounds hb;
  if (given_bounds) {  // the caller read them back with its own results
    std::memcpy(&hb, given_bounds, sizeof(Bounds));
  } else {
    hipLaunchKernelGGL(k_bounds<D>, dim3(nbb), dim3(kBlock), 0, st, x, y, z, stride, t, n,
                       d_part, (const int64_t*)nullptr);
    hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(kBlock), 0, st, d_part, nbb, d_b);
    RPT_CHECK_LAUNCH();
    RPT_HIP(hipMemcpyAsync(&hb, d_b, sizeof(Bounds), hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
  }
  tm.mark();
  if (hb.nonfinite_xyz) {
    set_error("Input contains NaN or infinity in coordinates");
    return RPT_ENONFINITE;
  }
  const float epst = (float)eps_time;
  g = Geom{};
  g.eps2 = eps_space * eps_space;
  g.epst = epst;
  const bool screen = ab().f32_screen && g.eps2 >= 1e-20 && g.eps2 <= 1e30;
  g.e2lo = screen ? (float)(g.eps2 * (1.0 - 1e-5)) : -1.0f;
  g.e2hi = screen ? (float)(g.eps2 * (1.0 + 1e-5)) : INFINITY;
  g.min_samples = min_samples;
  double lo[4], hi[4];
  for (int k = 0; k < 4; ++k) {
    lo[k] = (double)ord2f(hb.mn[k]);
    hi[k] = (double)ord2f(hb.mx[k]);
  }
  if (hb.n_finite_t == 0) lo[3] = hi[3] = 0.0;
  integral_t = !hb.nonintegral_t;
  const double margin = 1.0 + 1.0 / 1048576.0;  // 2^-20
  // cell side: >= eps/2 keeps every neighbour within +-2 cells; in 2-D up to eps/sqrt(2) keeps a
  // full cell's diagonal within eps (mutual cells possible), and larger cells hold more points,
  // so more of them are decided whole: 0.7 eps in 2-D (1000-frame stack 12.86 -> 12.41 ms, the
  // dense share's K5 0.66 -> 0.84 of roofline, same box); ab().cell_side overrides (0.5 - 0.7)
  const double sf = (D == 2) ? ab().cell_side : 0.5;
  double cs = (eps_space > 0.0 ? eps_space * sf : 1.0) * margin;
  double ct = !hb.nonintegral_t ? 1.0 : (epst > 0.f ? (double)epst : 1.0) * margin;
  const int64_t cmax = std::min<int64_t>(std::max<int64_t>(int64_t(1) << 22, 4 * n),
                                         int64_t(1) << 30);
  auto dims = [&](double ext, double side) -> int64_t {
    const double q = floor(ext / side) + 1.0;
    return q > 1e9 ? (int64_t)1e9 : (int64_t)q;
  };
  int64_t nx = 1, ny = 1, nz = 1;
  for (int it = 0; it < 200; ++it) {
    nx = dims(hi[0] - lo[0], cs);
    ny = dims(hi[1] - lo[1], cs);
    nz = (D == 3) ? dims(hi[2] - lo[2], cs) : 1;
    nt = dims(hi[3] - lo[3], ct);
    if ((double)nx * ny * nz * nt <= (double)cmax) break;
    if ((double)nt > (double)nx * ny * nz)
      ct *= 2.0;
    else
      cs *= 2.0;
  }
  g.ox = lo[0];
  g.oy = lo[1];
  g.oz = lo[2];
  g.ot = lo[3];
  g.cs = cs;
  g.ct = ct;
  g.inv_cs = 1.0 / cs;
  g.inv_ct = 1.0 / ct;
  g.nx = (int)nx;
  g.ny = (int)ny;
  g.nz = (int)nz;
  g.nt = (int)nt;
  g.cells = nx * ny * nz * nt;
  g.fnx.init((uint32_t)nx);
  g.fny.init((uint32_t)ny);
  g.fnz.init((uint32_t)nz);
  g.fslab.init((uint32_t)(nx * ny * nz));
  {
    const double r = slab_reach();  // (infinite for an infinite eps_time: generic windows)
    g.rt = (integral_t && r < 1e9) ? (int)std::min(r, (double)nt) : -1;
    g.tfree = (g.rt >= 0 && ct == 1.0 && (double)g.rt <= std::floor((double)epst)) ? 1 : 0;
  }
  // a slab is one time value and a cell's diagonal is within eps (margin far above the rounding
  // of the cell index and of k_cell_box's d2 <= eps2 test), so a cell's points are pairwise
  // adjacent; a coarsened cell side (cs doubled) fails 2 cs^2 <= eps^2
  all_mutual = D == 2 && integral_t && ct == 1.0 && hb.n_finite_t == n && min_samples >= 1 &&
               epst >= 0.f && eps_space > 0.0 && 2.0 * cs * cs <= g.eps2 * (1.0 - 1e-6);
  C = g.cells;
  const int64_t C1 = C + 1;  // + the isolated cell (non-finite t)
  Budget bud;
  bud.add<Bounds>(1);
  for (int k = 0; k < 4; ++k) bud.add<uint32_t>(n);  // keys, vals, alt
  bud.add<int64_t>(radix_tmp_elems(n));
  bud.add<float4>(n);
  bud.add<int32_t>(n);       // sorig
  bud.add<int32_t>(n);       // skey
  bud.add<int32_t>(C1 + 1);  // cell_start
  bud.add<int64_t>(scan_tmp_elems(C1 + 1) + scan_tmp_elems(n + 1));
  bud.add<uint8_t>(C1);
  bud.add<int32_t>(C1);  // rep
  bud.add<float2>(nt);
  bud.add<uint8_t>(n);      // core
  bud.add<int32_t>(n);      // parent
  bud.add<int32_t>(n);      // ccmin
  bud.add<int32_t>(n + 1);  // cid
  bud.add<int32_t>(n + 1);  // non-core list (+count)
  bud.add<int32_t>(n);      // slab (global finalize; denoise: orig -> sorted)
  bud.add<uint8_t>(C1);     // fok (denoise)
  bud.add<int32_t>(C1);     // cell_min
  bud.add<int32_t>(C1);     // cell_root
  bud.add<uint64_t>(C1);    // cell_min_pair (union star initialisation)
  bud.add<uint32_t>(n / 32 + 1);  // min_bits
  bud.add<int32_t>(n / 32 + 2);   // min_pref
  bud.add<int32_t>(n + 1);  // occ
  bud.add<int32_t>(n + 1);  // hpos
  bud.add<CellRec<D>>(C1);  // crec
  bud.add<uint32_t>(C1 / 32 + 2);  // occupancy bits
  bud.add<uint32_t>(C1 / 32 + 2);  // core_bits
  bud.add<uint32_t>(C1 / 32 + 2);  // near_bits
  bud.add<int32_t>(nt + 1);        // slab_lo (slab-bucket path)
  bud.add<int32_t>(nt + 1);        // slab_occ (slab-bucket path)
  bud.add<int32_t>(nt + 1);        // occ_base (slab-bucket path)
  bud.add<int32_t>((size_t)(ny * nz * nt) + 1);  // rowq (LDS-tile passes)
  bud.add<int32_t>((size_t)(ny * nz * nt) + 1);  // row counts
  bud.add<int32_t>(n);  // counts (count_pass; kept through a min_samples sweep)
  RPT_TRY(arena.reserve(bud.bytes, st));
  (void)arena.carve_n<Bounds>(1);
  uint32_t* keys = arena.carve_n<uint32_t>(n);
  uint32_t* vals = arena.carve_n<uint32_t>(n);
  uint32_t* keys_alt = arena.carve_n<uint32_t>(n);
  uint32_t* vals_alt = arena.carve_n<uint32_t>(n);
  pmask = reinterpret_cast<uint4*>(keys);  // 4 x n u32, contiguous: room for n_occ <= n masks
  int64_t* rtmp = arena.carve_n<int64_t>(radix_tmp_elems(n));
  pts = arena.carve_n<float4>(n);
  sorig = arena.carve_n<int32_t>(n);
  skey = arena.carve_n<int32_t>(n);
  cell_start = arena.carve_n<int32_t>(C1 + 1);
  stmp = arena.carve_n<int64_t>(scan_tmp_elems(C1 + 1) + scan_tmp_elems(n + 1));
  mutual = arena.carve_n<uint8_t>(C1);
  rep = arena.carve_n<int32_t>(C1);
  slab_t = arena.carve_n<float2>(nt);
  core = arena.carve_n<uint8_t>(n);
  parent = arena.carve_n<int32_t>(n);
  ccmin = arena.carve_n<int32_t>(n);
  cid = arena.carve_n<int32_t>(n + 1);
  nc_list = arena.carve_n<int32_t>(n + 1);
  slab = arena.carve_n<int32_t>(n);
  fok = arena.carve_n<uint8_t>(C1);
  cell_min = arena.carve_n<int32_t>(C1);
  cell_root = arena.carve_n<int32_t>(C1);
  cell_min_pair = arena.carve_n<uint64_t>(C1);
  min_bits = arena.carve_n<uint32_t>(n / 32 + 1);
  min_pref = arena.carve_n<int32_t>(n / 32 + 2);
  occ = arena.carve_n<int32_t>(n + 1);
  hpos = arena.carve_n<int32_t>(n + 1);
  CellRec<D>* cr = arena.carve_n<CellRec<D>>(C1);
  crec = cr;
  occ_bits = arena.carve_n<uint32_t>(C1 / 32 + 2);  // +1: two-word window reads
  core_bits = arena.carve_n<uint32_t>(C1 / 32 + 2);
  near_bits = arena.carve_n<uint32_t>(C1 / 32 + 2);
  int32_t* slab_lo = arena.carve_n<int32_t>(nt + 1);
  int32_t* slab_occ = arena.carve_n<int32_t>(nt + 1);
  int32_t* occ_base = arena.carve_n<int32_t>(nt + 1);
  rowq = arena.carve_n<int32_t>((size_t)(ny * nz * nt) + 1);
  rowcnt = arena.carve_n<int32_t>((size_t)(ny * nz * nt) + 1);
  counts = arena.carve_n<int32_t>(n);
  rowq_ok = false;
  if (!slab_lo || !rowcnt || !counts) {
    set_error("internal: scratch carve overflow");
    return RPT_ENOMEM;
  }
  // time-ordered finite 2-D points with a slab's cells fitting LDS: per-slab counting sort
  bucket_allmin = false;
  const bool bucket = ab().k4_bucket && D == 2 && hb.n_finite_t == n && !hb.t_descends &&
                      (int64_t)nx * ny <= kBucketCells && nt < (int64_t(1) << 31);
  // xy points: written by the slab writers only, every time finite (no isolated cell)
  xy_points = may_xy && bucket && D == 2 && hb.n_finite_t == n && xy_rule();
  // (xy points: the writer fills slab_t from the slabs' own time values)
  float2* const slab_t_w = xy_points ? slab_t : nullptr;
  if (bucket) {
    hipLaunchKernelGGL(k_slab_lo, dim3(grid_for(64 * (nt + 1), kBlock, 4096)), dim3(kBlock), 0,
                       st, t, n, g, slab_lo, occ_bits, (int64_t)(C1 / 32 + 2));
    // the slabs write their occupied cells (ascending) into hpos at their point offsets, the
    // occupancy bits and their counts; one scan over the slabs and a gather give the list
    const size_t hist_bytes = sizeof(int32_t) * (size_t)nx * ny;
    // blocks per slab (measured, same box): dense slabs (> 128 k points) split into ~kChunkPts
    // point chunks (configs[4] share: grid 2.93 -> 2.04 ms); short stacks split until ~512 blocks
    // fill the GPU (125 frames: 0.193 -> 0.177 ms); 1000 standard slabs stay one block each
    // (three chunks measured 1.10 -> 1.25 ms).  The chunk histograms live in the radix key
    // buffers (4 n words, dead on this path).
    const int64_t avg = n / std::max<int64_t>(nt, 1);
    // dense slabs: the label passes' scattered core-label writes cost more than the inverse
    // permutation written here (configs[4] share: 676 -> 253 us for +57 in the scatter; at
    // standard density the scattered writes stay in L2 and the extra store costs +68 us)
    dense_slabs = avg > 8 * kChunkPts;
    spos_on = ab().label_orig == 2 || (ab().label_orig == 1 && dense_slabs);
    int32_t* spos_w = spos_on ? slab : nullptr;
    int64_t ch = avg > 8 * kChunkPts ? (avg + kChunkPts - 1) / kChunkPts : 1;
    ch = std::max<int64_t>(ch, (512 + nt - 1) / std::max<int64_t>(nt, 1));
    int CH = (int)std::min<int64_t>(ch, 64);
    while (CH > 1 && (int64_t)nt * CH * nx * ny > 4 * n) --CH;
    if (ab().slab_chunks > 0) CH = ab().slab_chunks;
    const bool coalesced_scan = CH >= 8 && (int64_t)nt * CH * nx * ny <= 4 * n &&
                                !ab().chunk_scan;
    if (CH > 1 && (int64_t)nt * CH * nx * ny <= 4 * n) {
      int32_t* hist_g = reinterpret_cast<int32_t*>(keys);
      // the coalesced passes pay for their extra launches only with many chunks per slab (dense
      // slabs: configs[4] share 357 -> 115 us); a few chunks per slab (short standard stacks,
      // split to fill the GPU) keep the one-block-per-slab scan (125 frames: 38 vs 53 us)
      RPT_HIP(hipFuncSetAttribute((const void*)k_slab_chunk_hist,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_bytes));
      const void* scatter = with_bool(
          xy_points, [](auto xy) { return (const void*)k_slab_chunk_scatter<xy.value>; });
      RPT_HIP(hipFuncSetAttribute(scatter, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)hist_bytes));
      hipLaunchKernelGGL(k_slab_chunk_hist, dim3((unsigned)(nt * CH)), dim3(kBucketBlock),
                         hist_bytes, st, x, y, stride, g, slab_lo, CH, hist_g);
      if (!coalesced_scan) {
        hipLaunchKernelGGL(k_slab_chunk_scan, dim3((unsigned)nt), dim3(kBucketBlock), 0, st, g,
                           slab_lo, CH, hist_g, cell_start, hpos, slab_occ, occ_bits);
      } else {
        // cell_start, cursors, occupancy from coalesced passes; the flags and their positions in
        // cell_min / cell_root (C1 words each, first written after the grid build)
        const int64_t cells = (int64_t)nt * nx * ny;
        const int P = (int)(nx * ny);
        const int gc = grid_for(cells, kBlock, 8192);
        hipLaunchKernelGGL(k_chunk_totals, dim3(gc), dim3(kBlock), 0, st, hist_g, cells, P, CH,
                           cell_start);
        RPT_TRY(exclusive_scan_total_i32(cell_start, cell_start, cells, st));
        hipLaunchKernelGGL(k_chunk_cursors, dim3(gc), dim3(kBlock), 0, st, hist_g, cells, P, CH,
                           cell_start, slab_lo, occ_bits, cell_min);
        RPT_TRY(exclusive_scan_total_i32(cell_min, cell_root, cells, st));
        hipLaunchKernelGGL(k_occ_write, dim3(gc), dim3(kBlock), 0, st, cell_min, cell_root,
                           cells, occ);
        hipLaunchKernelGGL(k_cell_start_end, dim3(1), dim3(64), 0, st, cell_start, cells);
        hipLaunchKernelGGL(k_slab_occ_base, dim3(grid_for(nt + 1, kBlock, 1024)), dim3(kBlock), 0,
                           st, cell_root, P, nt, occ_base);
        RPT_CHECK_LAUNCH();
      }
      with_bool(xy_points, [&](auto xy) {
        hipLaunchKernelGGL(k_slab_chunk_scatter<xy.value>, dim3((unsigned)(nt * CH)),
                           dim3(kBucketBlock), hist_bytes, st, x, y, stride, t, g, slab_lo, CH,
                           hist_g, points<xy.value>(), sorig, skey, spos_w, slab_t_w);
      });
    } else {
      // the fused K5's all-core cell minima from the counting sort when both LDS arrays fit 64 KiB
      bucket_allmin = k5_fused_path() && 2 * hist_bytes <= 65536 &&
                      ab().bucket_allmin != 0;  // (=0: from k_cell_box; A/B)
      const size_t lds = bucket_allmin ? 2 * hist_bytes : hist_bytes;
      const void* bucket_fn =
          with_bool(xy_points, [](auto xy) { return (const void*)k_slab_bucket<xy.value>; });
      RPT_HIP(hipFuncSetAttribute(bucket_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
#ifdef RPT_AB
      if (ab().stats) {  // A/B diagnostics: blocks per CU the runtime admits
        int nb = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, bucket_fn, kBucketBlock, lds);
        std::fprintf(stderr, "[rpt stats] slab_bucket lds=%zu nx=%d ny=%d blocks_per_cu=%d\n", lds,
                     (int)nx, (int)ny, nb);
      }
#endif
      auto* cmin_all =
          bucket_allmin ? reinterpret_cast<unsigned long long*>(cell_min_pair) : nullptr;
      with_bool(xy_points, [&](auto xy) {
        hipLaunchKernelGGL(k_slab_bucket<xy.value>, dim3((unsigned)nt), dim3(kBucketBlock), lds,
                           st, x, y, stride, t, g, slab_lo, points<xy.value>(), sorig, skey,
                           spos_w, cell_start, hpos, slab_occ, occ_bits, cmin_all, slab_t_w);
      });
    }
    RPT_CHECK_LAUNCH();
    if (coalesced_scan) {
      n_occ_dev = occ_base + nt;  // the occupied list is written already
    } else {
      RPT_TRY(exclusive_scan_total_i32(slab_occ, occ_base, nt, st));
      hipLaunchKernelGGL(k_occ_gather, dim3((unsigned)nt), dim3(kBlock), 0, st, hpos, slab_lo,
                         occ_base, occ);
      RPT_CHECK_LAUNCH();
      n_occ_dev = occ_base + nt;
    }
  } else {
    hipLaunchKernelGGL(k_keys<D>, dim3(gb), dim3(kBlock), 0, st, x, y, z, stride, t, n, g, keys,
                       vals);
    RPT_CHECK_LAUNCH();
    int bits = 1;
    while ((int64_t(1) << bits) <= C1) ++bits;
    uint32_t *sk, *sv;
    RPT_TRY(radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, bits, rtmp, &sk, &sv, st));
    dense_slabs = false;
    spos_on = ab().label_orig == 2;
    hipLaunchKernelGGL(k_gather<D>, dim3(gb), dim3(kBlock), 0, st, x, y, z, stride, t, n, sk, sv,
                       pts, sorig, skey, spos_on ? slab : nullptr);
    RPT_HIP(hipMemsetAsync(cell_start, 0, sizeof(int32_t) * C1, st));
    hipLaunchKernelGGL(k_cell_runs, dim3(gb), dim3(kBlock), 0, st, skey, n, cell_start, hpos);
    RPT_CHECK_LAUNCH();
    RPT_TRY(exclusive_scan_total_i32(cell_start, cell_start, C1, st));
    RPT_TRY(exclusive_scan_total_i32(hpos, hpos, n, st));
    RPT_HIP(hipMemsetAsync(occ_bits, 0, sizeof(uint32_t) * (C1 / 32 + 2), st));
    hipLaunchKernelGGL(k_occ_list, dim3(gb), dim3(kBlock), 0, st, skey, n, hpos, occ, occ_bits);
    RPT_CHECK_LAUNCH();
    n_occ_dev = hpos + n;
  }
  {
    auto* cmin_w = bucket_allmin ? nullptr : reinterpret_cast<unsigned long long*>(cell_min_pair);
    const int32_t* so_w = (k5_fused_path() && !bucket_allmin) ? (const int32_t*)sorig : nullptr;
    // small cells one lane each on large standard-density stacks (1000 frames: 346 -> 273 us);
    // the 125-frame share has too few 64-cell waves to fill the GPU (48 -> 60 us) and dense
    // slabs' cells are large (324 -> 402 us): 16 lanes for every cell there
    // (RPT_CELL_BOX_MIXED=0 in the A/B build: always)
    const bool mixed = ab().cell_box_mixed == 2 ||
                       (ab().cell_box_mixed == 1 && !dense_slabs && n > (int64_t(1) << 24));
    const dim3 gm(grid_for(n, kBlock, 4096)), gl(grid_for(kCbLanes * n, kBlock, 8192));
    with_bool(xy_points, [&](auto xy) {
      constexpr bool XY = decltype(xy)::value;
      if constexpr (D == 2 || !XY) {  // (xy points are 2-D: no <3, true> form)
        // XY: the records' time fields from slab_t, written above
        const float2* slab_t_r = XY ? slab_t : nullptr;
        if (mixed)
          hipLaunchKernelGGL((k_cell_box_mixed<D, XY>), gm, dim3(kBlock), 0, st, points<XY>(),
                             cell_start, occ, n_occ_dev, g, mutual, cr, cmin_w, so_w, slab_t_r);
        else
          hipLaunchKernelGGL((k_cell_box<D, XY>), gl, dim3(kBlock), 0, st, points<XY>(),
                             cell_start, occ, n_occ_dev, g, mutual, cr, cmin_w, so_w, slab_t_r);
      }
    });
  }
  RPT_CHECK_LAUNCH();
  // (xy points: the writer filled slab_t from the slabs' own time values)
  if (!xy_points)
    hipLaunchKernelGGL(k_slab_range<D>, dim3((unsigned)nt), dim3(kBlock), 0, st, cr, occ, hpos,
                       cell_start, (int64_t)(C / nt), (int)nt, slab_t,
                       bucket ? occ_base : nullptr);
  RPT_CHECK_LAUNCH();
  tm.mark();
  return RPT_OK;
}

int32_t DbscanState::build(const float* x, const float* y, const float* z, int64_t stride,
                           const float* t, int64_t n_, double eps_space, double eps_time,
                           int32_t ms, bool timing, hipStream_t st) {
  n = n_;
  dim = z ? 3 : 2;
  min_samples = ms;
  xy_points = false;
  struct Consume {  // the caller's promise covers this build only
    bool& f;
    ~Consume() { f = false; }
  } consume{may_xy};
  tm.start(timing, st);
  degenerate = !(eps_space >= 0.0) || !((float)eps_time >= 0.0f);
  if (degenerate) return RPT_OK;
  return dim == 2 ? build_t<2>(x, y, z, stride, t, eps_space, eps_time, st)
                  : build_t<3>(x, y, z, stride, t, eps_space, eps_time, st);
}

int32_t DbscanState::core_pass(hipStream_t st) {
  cmin_ready = false;
  if (degenerate) return RPT_OK;
  // cflag lives in rep (int32 per cell, rebuilt by union_pass); the cell queue in ccmin and the
  // point queue in nc_list (both rebuilt later), counters in cid[n] / nc_list[n]
  int32_t* cflag = rep;
  int32_t* cq = ccmin;
  int32_t* n_cq = cid + n;
  int32_t* slow = nc_list;
  int32_t* n_slow = nc_list + n;
  const int32_t* n_occ = n_occ_dev;
  const double rs = slab_reach();
  const bool oct = oct_ok();
  // k_core_cells_oct's grid: eight lanes per occupied cell (at most n), a multiple of 8 blocks
  const dim3 g_oct((grid_for(8 * n, kBlock, 8192) + 7) & ~7);
  if (!k5_fused_path()) RPT_TRY(need_float4("core_pass"));
#ifdef RPT_AB  // A/B-only forms (stdbscan_ab.inc)
  if (oct && ab().k5_tiles) {
    // LDS tiles: band height BY with the map (W slabs x BY + 4 rows x nx) and the undecided list
    // (BY x nx own cells) within their LDS arrays; rowq (kept for the label pass's tiles)
    const int R = (int)rs, W = 2 * R + 1;
    const int by = std::min({8, kTileMap / (W * g.nx) - 4, kTileUnd / g.nx});
    const int64_t nrows = (int64_t)g.nt * g.ny;
    if (by >= 1) {
      hipLaunchKernelGGL(k_row_occ, dim3(grid_for(nrows, kBlock, 4096)), dim3(kBlock), 0, st,
                         occ_bits, nrows, g.nx, rowcnt);
      RPT_CHECK_LAUNCH();
      RPT_TRY(exclusive_scan_total_i32(rowcnt, rowq, nrows, st));
      rowq_ok = true;
      const int nbands = (g.ny + by - 1) / by;
      tile_by = by;
      tile_nbands = nbands;
      tile_R = R;
      const int64_t ntiles = (int64_t)g.nt * nbands;
      const unsigned grid = (unsigned)(((ntiles + 1) + 7) & ~(int64_t)7);
      hipLaunchKernelGGL(k_core_tiles, dim3(grid), dim3(kTileBlock), 0, st, g, R, by, nbands,
                         ntiles, occ, n_occ, rowq, rec<2>(), mutual, occ_bits, slab_t, pts, core);
      RPT_CHECK_LAUNCH();
      tm.mark();
      return RPT_OK;
    }
  }
  if (ab().k5_mode != 0) {
    const bool k5_fill = ab().k5_mode == 2;  // (no queue: the cells' point flags by a fill pass)
    // cells decide (and write their points' flags) in one pass; the undecided cells' points are
    // settled by k_core_slow_cells, which walks the occupied cells itself (no queue, no fill)
    if (oct) {
      hipLaunchKernelGGL(k_core_cells_oct<false>, g_oct, dim3(kBlock), 0, st, g, (int)rs, occ,
                         n_occ, rec<2>(), mutual, occ_bits, slab_t, cflag, (int32_t*)nullptr,
                         k5_fill ? (uint8_t*)nullptr : core);
      if (k5_fill)
        hipLaunchKernelGGL(k_core_fill<false>, dim3(tile_grid(n)), dim3(kBlock), 0, st, skey, n,
                           cflag, core, slow, n_slow);
    } else {
      RPT_TRY(zero_n(st, 1, &n_cq));
      hipLaunchKernelGGL(k_core_cell_fast, dim3(tile_grid(n)), dim3(kBlock), 0, st, occ, n_occ,
                         g, cell_start, mutual, cflag, cq, n_cq);
      with_dim(dim, [&](auto d) {
        hipLaunchKernelGGL(k_core_cell_window<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st,
                           g, occ, rec<d.value>(), occ_bits, slab_t, cq, n_cq, cflag);
      });
      hipLaunchKernelGGL(k_core_fill<false>, dim3(tile_grid(n)), dim3(kBlock), 0, st, skey, n,
                         cflag, core, slow, n_slow);
    }
    with_dim(dim, [&](auto d) {
      hipLaunchKernelGGL(k_core_slow_cells<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts,
                         g, rec<d.value>(), occ_bits, slab_t, occ, n_occ, cflag, core);
    });
    RPT_CHECK_LAUNCH();
    tm.mark();
    return RPT_OK;
  }
#endif
  // oct: the union's per-cell minima (cell_min_pair) come out of the fill and slow passes
  auto* cm = oct ? reinterpret_cast<unsigned long long*>(cell_min_pair) : nullptr;
  if (k5_fused_path()) {
    RPT_TRY(zero_n(st, 1, &n_slow));
    // the cell pass's decisions handed to the slow pass when its window's 5 W (slab, row) pairs
    // x 5 columns fit a 128-bit mask (W <= 5; pmask / clo per occupied cell in the dead radix
    // buffers / cid, both rebuilt later)
    const bool masked = (int)rs <= 2 && ab().k5_mask;
    if (!masked) RPT_TRY(need_float4("core_pass"));
    uint4* k5m = reinterpret_cast<uint4*>(pmask);
    if (masked) {
      hipLaunchKernelGGL((k_core_cells_oct<true, true>), g_oct, dim3(kBlock), 0, st, g, (int)rs,
                         occ, n_occ, rec<2>(), mutual, occ_bits, slab_t, (int32_t*)nullptr,
                         (int32_t*)nullptr, core, cm, slow, cq, n_slow, k5m, cid);
      with_bool(xy_points, [&](auto xy) {
        hipLaunchKernelGGL(k_core_slow_masked<xy.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st,
                           points<xy.value>(), g, (int)rs, rec<2>(), occ, slow, cq, n_slow, k5m,
                           cid, core, sorig, cm);
      });
    } else {
      hipLaunchKernelGGL(k_core_cells_oct<true>, g_oct, dim3(kBlock), 0, st, g, (int)rs, occ,
                         n_occ, rec<2>(), mutual, occ_bits, slab_t, (int32_t*)nullptr,
                         (int32_t*)nullptr, core, cm, slow, cq, n_slow);
      if (g.rt >= 0 && (2 * g.rt + 1) * 25 <= 128)
        hipLaunchKernelGGL((k_core_slow<2, 2>), dim3(wave_grid(n)), dim3(kBlock), 0, st, pts,
                           skey, g, rec<2>(), occ_bits, slab_t, slow, n_slow, core, sorig, cm, cq);
      else
        hipLaunchKernelGGL(k_core_slow<2>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey, g,
                           rec<2>(), occ_bits, slab_t, slow, n_slow, core, sorig, cm, cq);
    }
    RPT_CHECK_LAUNCH();
    cmin_ready = true;
#ifdef RPT_AB
    if (ab().stats) {  // A/B diagnostics: K5's slow queue and its cells (syncs)
      int32_t h = 0;
      (void)hipMemcpyAsync(&h, n_slow, 4, hipMemcpyDeviceToHost, st);
      (void)hipStreamSynchronize(st);
      std::vector<int32_t> keys((size_t)std::max(h, 0));
      if (h > 0) (void)hipMemcpy(keys.data(), cq, sizeof(int32_t) * (size_t)h, hipMemcpyDeviceToHost);
      std::sort(keys.begin(), keys.end());
      int64_t distinct = 0, max_run = 0, run = 0;
      for (size_t i = 0; i < keys.size(); ++i) {
        run = (i > 0 && keys[i] == keys[i - 1]) ? run + 1 : 1;
        if (run == 1) ++distinct;
        max_run = std::max(max_run, run);
      }
      std::fprintf(stderr, "[rpt stats] n=%lld k5_slow_queue=%d cells=%lld max_per_cell=%lld\n",
                   (long long)n, h, (long long)distinct, (long long)max_run);
    }
#endif
    tm.mark();
    return RPT_OK;
  }
  if (oct) {
    hipLaunchKernelGGL(k_core_cells_oct<false>, g_oct, dim3(kBlock), 0, st, g, (int)rs, occ, n_occ,
                       rec<2>(), mutual, occ_bits, slab_t, cflag, n_slow, (uint8_t*)nullptr);
  } else {
    RPT_TRY(zero_n(st, 1, &n_slow));
    RPT_TRY(zero_n(st, 1, &n_cq));
    hipLaunchKernelGGL(k_core_cell_fast, dim3(tile_grid(n)), dim3(kBlock), 0, st, occ, n_occ, g,
                       cell_start, mutual, cflag, cq, n_cq);
    with_dim(dim, [&](auto d) {
      hipLaunchKernelGGL(k_core_cell_window<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st, g,
                         occ, rec<d.value>(), occ_bits, slab_t, cq, n_cq, cflag);
    });
  }
  hipLaunchKernelGGL(k_core_fill<true>, dim3(tile_grid(n)), dim3(kBlock), 0, st, skey, n, cflag,
                     core, slow, n_slow, sorig, cm, C);
  // (a pair, not with_dim: the 2-D form passes sorig whether or not cm is set, the 3-D form none)
  if (dim == 2)
    hipLaunchKernelGGL(k_core_slow<2>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey, g,
                       rec<2>(), occ_bits, slab_t, slow, n_slow, core, sorig, cm);
  else
    hipLaunchKernelGGL(k_core_slow<3>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey, g,
                       rec<3>(), occ_bits, slab_t, slow, n_slow, core);
  RPT_CHECK_LAUNCH();
  cmin_ready = cm != nullptr;
  tm.mark();
  return RPT_OK;
}

int32_t DbscanState::count_pass(int32_t* counts_sorted, hipStream_t st) {
  if (degenerate) return RPT_OK;  // (no grid: the callers write zeros)
  RPT_TRY(need_float4("count_pass"));
  with_dim(dim, [&](auto d) {
    hipLaunchKernelGGL(k_count_cells<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, g,
                       occ, n_occ_dev, rec<d.value>(), occ_bits, slab_t, counts_sorted);
  });
  RPT_CHECK_LAUNCH();
  tm.mark();
  return RPT_OK;
}

int32_t DbscanState::core_from_counts(const int32_t* counts_sorted, int32_t m, hipStream_t st) {
  if (m < 1) {  // build_t's all_mutual and labels_local's branches depend on the sign
    set_error("core_from_counts: min_samples must be >= 1");
    return RPT_EINVAL;
  }
  min_samples = g.min_samples = m;
  cmin_ready = false;  // no core pass filled the cell minima for these flags
  if (degenerate) return RPT_OK;
  RPT_TRY(zero_n(st, 1, &n_core_dev));
  hipLaunchKernelGGL(k_core_from_counts, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st,
                     counts_sorted, n, m, core, n_core_dev);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t DbscanState::union_pass(hipStream_t st, bool fused) {
  cell_comp = false;
  if (degenerate) return RPT_OK;
  const AbSwitches& a = ab();
  const int uf_flags = a.uf_flags;  // see XcdRange
  const int gb = grid_for(n, kBlock, 2048);
  const int gw = wave_grid(n);
  const unsigned gp = (unsigned)((n + kBlock - 1) / kBlock);
  const int32_t* n_occ = n_occ_dev;
  // per-cell (min original index, sorted index) of the core points, one u64 per cell
  auto* cmin = reinterpret_cast<unsigned long long*>(cell_min_pair);
  // 2-D: the first union pass lists its cells with undecided candidates in nc_list (free until
  // the label pass), their count at nc_list[n] (zeroed by k_init_occ_cells)
  const bool listing = a.union_list && dim == 2;
  int32_t* plist = listing ? nc_list : nullptr;
  int32_t* pcount = listing ? nc_list + n : nullptr;
  // 2-D pair path: the non-mutual cells with core points listed by the first pass in cid (free
  // until the label pass), their count at cid[n]; k_union_nm then takes only their points
  // (RPT_UNION_NM=0 in the A/B build: k_union over every point)
  const bool nm = dim == 2 && a.union_pair && a.union_nm;
  int32_t* nm_list = nm ? cid : nullptr;
  int32_t* nm_count = nm ? cid + n : nullptr;
  // all_mutual grids on the default 2-D pair path: only the cell representatives' parent
  // entries are read from here to the label stage (k_union_cells_pair, k_cell_root_snapshot and
  // k_union_listed start every walk at rep[c]; k_union_nm, which walks the points of non-mutual
  // cells, has nothing listed and is not launched), so the star initialisation is per cell
  // (not with the A/B label tiles, which read ccmin, nor with the A/B compression pass:
  // k_compress walks EVERY core point's parent chain, so it keeps the per-point init)
  cell_comp = fused && cell_comp_ok();
  // (xy points: only the per-cell path's kernels below know the layout)
  if (!cell_comp) RPT_TRY(need_float4("union_pass"));
  // the per-cell minima: from the core pass (cmin_ready) or from the final core flags here
  if (!cell_comp || !cmin_ready)
    hipLaunchKernelGGL(k_init_occ_cells, dim3(gb), dim3(kBlock), 0, st, occ, n_occ, C, rep,
                       cmin_ready ? nullptr : cmin, pcount, nm_count);
  if (!cmin_ready)
    hipLaunchKernelGGL(k_cell_min_pair, dim3(gb), dim3(kBlock), 0, st, skey, core, sorig, n, C,
                       cmin);
  if (cell_comp)
    hipLaunchKernelGGL(k_parent_init_cells, dim3(gb), dim3(kBlock), 0, st, C, cmin, rep, parent,
                       pcount, nm_count, min_bits, min_words(),
                       near_bits_ok() ? (int32_t*)nullptr : cell_min, occ_bits, core_bits,
                       (int64_t)((C + 1) / 32 + 2));
  else
    hipLaunchKernelGGL(k_parent_init_pair, dim3(grid_for(n, kBlock * kPU, 2048)), dim3(kBlock), 0,
                       st, parent, n, core, skey, mutual, cmin, C, rep);
  int32_t* lstat_dev = nullptr;  // (A/B diagnostics)
  if (dim == 2) {
    uint4* pm = listing ? pmask : nullptr;
    if (a.union_pair && cell_comp)  // candidates by core_bits, no mutual[] per candidate
      hipLaunchKernelGGL(k_union_cells_pair<true>, dim3(gw), dim3(kBlock), 0, st, pts, g, occ,
                         n_occ, rec<2>(), core_bits, slab_t, rep, mutual, sorig, parent, uf_flags,
                         pm, plist, pcount, union_cpw(), nm_list, nm_count);
    else if (a.union_pair)  // two cells per wave (RPT_UNION_PAIR=0 in the A/B build: one)
      hipLaunchKernelGGL(k_union_cells_pair<false>, dim3(gw), dim3(kBlock), 0, st, pts, g, occ,
                         n_occ, rec<2>(), occ_bits, slab_t, rep, mutual, sorig, parent, uf_flags,
                         pm, plist, pcount, union_cpw(), nm_list, nm_count);
    else
      hipLaunchKernelGGL((k_union_cells<2, false>), dim3(gw), dim3(kBlock), 0, st, pts, g,
                         cell_start, occ, n_occ, rec<2>(), occ_bits, slab_t, core, rep, mutual,
                         sorig, parent, uf_flags, pm, plist, pcount);
#ifdef RPT_AB
    if (listing && ab().stats) {  // (A/B diagnostics: a leaked 16 B per process)
      static int32_t* buf = nullptr;
      if (!buf) (void)hipMalloc(&buf, 16);
      lstat_dev = buf;
      (void)hipMemsetAsync(lstat_dev, 0, 16, st);
    }
#endif
    if (listing) {
      // the snapshot in cell_root (free until the label stage's k_cell_roots); not on dense
      // slabs, where it measured slower (configs[4] share: +38 us snapshot, listed 867 -> 916 us;
      // 1000 standard frames: listed 348 -> 202 us for +28)
      const bool snap = ab().union_snap == 2 || (ab().union_snap == 1 && !dense_slabs);
      if (snap)
        hipLaunchKernelGGL(k_cell_root_snapshot, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock),
                           0, st, occ, n_occ, rep, parent, g.cells, uf_flags, cell_root);
      const int32_t* croot = snap ? (const int32_t*)cell_root : nullptr;
      with_bool(xy_points, [&](auto xy) {
        hipLaunchKernelGGL(k_union_listed<xy.value>, dim3(gw), dim3(kBlock), 0, st,
                           points<xy.value>(), g, occ, rec<2>(), occ_bits, slab_t, core, rep,
                           mutual, sorig, parent, uf_flags, pm, plist, pcount, croot, lstat_dev);
      });
    }
    else
      hipLaunchKernelGGL((k_union_cells<2, true>), dim3(gw), dim3(kBlock), 0, st, pts, g,
                         cell_start, occ, n_occ, rec<2>(), occ_bits, slab_t, core, rep, mutual,
                         sorig, parent, uf_flags, pm, plist, pcount);
    if (cell_comp) {
      // no non-mutual cell with core points (nm_count stays 0; k_label_core_cells checks it)
    } else if (nm)
      hipLaunchKernelGGL(k_union_nm<2>, dim3(gw), dim3(kBlock), 0, st, pts, g, cell_start,
                         rec<2>(), slab_t, core, rep, mutual, sorig, parent, nm_list, nm_count);
    else
      hipLaunchKernelGGL(k_union<2>, dim3(gp), dim3(kBlock), 0, st, pts, skey, n, g, cell_start,
                         rec<2>(), slab_t, core, rep, mutual, sorig, parent);
  } else {
    auto cells_pass = [&](auto partial) {  // (k_union_cells' PARTIAL: false, then true)
      hipLaunchKernelGGL((k_union_cells<3, partial.value>), dim3(gw), dim3(kBlock), 0, st, pts, g,
                         cell_start, occ, n_occ, rec<3>(), occ_bits, slab_t, core, rep, mutual,
                         sorig, parent, uf_flags);
    };
    cells_pass(std::false_type{});
    cells_pass(std::true_type{});
    hipLaunchKernelGGL(k_union<3>, dim3(gp), dim3(kBlock), 0, st, pts, skey, n, g, cell_start,
                       rec<3>(), slab_t, core, rep, mutual, sorig, parent);
  }
  RPT_CHECK_LAUNCH();
  // every later reader walks to the root with path halving (k_ccmin, k_comp_out, ...), so a
  // separate compression pass only moves that work; RPT_UF_COMPRESS=1 keeps it (A/B; read
  // above: it rules the per-cell init out)
#ifdef RPT_AB
  if (a.uf_compress && !cell_comp)
    hipLaunchKernelGGL(k_compress, dim3(gb), dim3(kBlock), 0, st, parent, core, n, sorig,
                       (int32_t*)nullptr);
  if (ab().stats) {  // A/B diagnostics: the queue and list sizes of this run (syncs)
    int32_t h[2] = {0, 0}, ls[4] = {0, 0, 0, 0};
    (void)hipMemcpyAsync(&h[0], n_occ_dev, 4, hipMemcpyDeviceToHost, st);
    if (listing) (void)hipMemcpyAsync(&h[1], pcount, 4, hipMemcpyDeviceToHost, st);
    if (lstat_dev) (void)hipMemcpyAsync(ls, lstat_dev, 16, hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    std::fprintf(stderr,
                 "[rpt stats] n=%lld occupied=%d listed_cells=%d listed: undecided=%d "
                 "roots_differ=%d searches=%d hits=%d\n",
                 (long long)n, h[0], h[1], ls[0], ls[1], ls[2], ls[3]);
    // the union init / component / core-label path of this run
    std::fprintf(stderr, "[rpt stats] n=%lld all_mutual=%d cell_comp=%d xy_points=%d\n",
                 (long long)n, all_mutual ? 1 : 0, cell_comp ? 1 : 0, xy_points ? 1 : 0);
  }
#endif
  RPT_CHECK_LAUNCH();
  tm.mark();
  return RPT_OK;
}

// component minima (k_ccmin; also queues the non-core points) -> MinRank prefix and cluster count
// cell_key (nullable, pre-filled with INT_MAX): also the per-cell smallest component key
int32_t DbscanState::cluster_ids(hipStream_t st, int32_t* cell_key, int32_t* zero) {
  const int64_t W = min_words();
  // per-cell roots of the mutual cells (read by k_ccmin for their core points); zero (nullable):
  // k_ccmin's non-core queue counter, cleared by k_cell_roots, which also clears the minimum
  // bits and fills cell_key (nullable) with INT_MAX (one launch instead of three)
  const bool cr = ab().cell_roots;
  if (cr) {
    hipLaunchKernelGGL(k_cell_roots, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st, parent,
                       occ, n_occ_dev, C, mutual, rep, cell_root, zero, min_bits, W, cell_key);
  } else {
    RPT_HIP(hipMemsetAsync(min_bits, 0, sizeof(uint32_t) * W, st));
    if (zero) RPT_HIP(hipMemsetAsync(zero, 0, sizeof(int32_t), st));
    if (cell_key)
      hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(C, kBlock, 8192)), dim3(kBlock), 0, st,
                         cell_key, C, INT_MAX);
  }
  hipLaunchKernelGGL(k_ccmin, dim3(tile_grid(n)), dim3(kBlock), 0, st, parent, core, n, sorig,
                     ccmin, min_bits, nc_list, nc_list + n, skey, mutual,
                     cr ? (const int32_t*)cell_root : nullptr, C, cell_key);
  hipLaunchKernelGGL(k_word_popc, dim3(grid_for(W, kBlock, 2048)), dim3(kBlock), 0, st, min_bits,
                     W, min_pref);
  RPT_CHECK_LAUNCH();
  return exclusive_scan_total_i32(min_pref, min_pref, W, st);
}

int32_t DbscanState::labels_local(int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st) {
  const int gb = grid_for(n, kBlock, 2048);
  if (degenerate) {
    hipLaunchKernelGGL(k_isolated_labels, dim3(gb), dim3(kBlock), 0, st, labels, n,
                       min_samples <= 0 ? 1 : 0);
    RPT_CHECK_LAUNCH();
    if (stats) {
      stats->n_points = n;
      stats->n_core = min_samples <= 0 ? n : 0;
      stats->n_clusters = min_samples <= 0 ? (int32_t)n : 0;
    }
    return RPT_OK;
  }
  int32_t* nc_count = nc_list + n;
  const MinRank mr{min_bits, min_pref};
  const unsigned glc = (unsigned)((grid_for(n, kBlock * kPU, 2048) + 7) & ~7);
  // the per-cell path by the core-cell bitmaps (core_bits written by k_parent_init_cells)
  const bool bits = cell_comp && core_bits_ok();
  const bool nearb = cell_comp && near_bits_ok();
  if (cell_comp) {
    // component ids per occupied cell (minimum bits and cell_min = INT_MAX cleared by
    // k_parent_init_cells), the rank prefix, then core labels + the non-core queue in one
    // per-point pass; ccmin is not written.  cid[n]: the union pass's non-mutual-cell count
    const int64_t W = min_words();
    if (nearb) {
      const int nbw = (int)((C + 1) / 32 + 2);
      hipLaunchKernelGGL(k_near_bits, dim3(grid_for(nbw, kBlock, 2048)), dim3(kBlock), 0, st,
                         core_bits, nbw, g.nx, g.ny, g.rt, near_bits);
    }
    hipLaunchKernelGGL(k_cell_comp, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st, parent,
                       occ, n_occ_dev, C, rep, sorig, cell_min, min_bits, nc_count);
    hipLaunchKernelGGL(k_word_popc, dim3(grid_for(W, kBlock, 2048)), dim3(kBlock), 0, st,
                       min_bits, W, min_pref);
    RPT_CHECK_LAUNCH();
    RPT_TRY(exclusive_scan_total_i32(min_pref, min_pref, W, st));
    with_bool(spos_on, [&](auto orig) {  // (ORIG: perm = spos, else sorig)
      with_bool(nearb, [&](auto nr) {
        hipLaunchKernelGGL((k_label_core_cells<orig.value, nr.value>), dim3(glc), dim3(kBlock), 0,
                           st, skey, core, orig.value ? slab : sorig, n, C, cell_min, mr, labels,
                           nc_list, nc_count, cid + n, n_clusters_ptr(),
                           nr.value ? (const uint32_t*)near_bits : nullptr);
      });
    });
  } else {
    // also the per-cell smallest keys (k_cell_min_key fused; cell_min filled with INT_MAX by
    // cluster_ids' first kernel) and nc_count cleared
    RPT_TRY(cluster_ids(st, cell_min, nc_count));
    if (spos_on)
      hipLaunchKernelGGL(k_label_core_orig, dim3(glc), dim3(kBlock), 0, st, ccmin, n, slab, mr,
                         labels);
    else
      hipLaunchKernelGGL(k_label_core, dim3(glc), dim3(kBlock), 0, st, ccmin, n, sorig, mr,
                         labels);
  }
  if (!cell_comp || ab().k7_w != 32 || use_label_tiles()) RPT_TRY(need_float4("labels_local"));
  int32_t* kstat = nullptr;  // (A/B diagnostics)
#ifdef RPT_AB
  if (ab().stats) {  // (a leaked 16 B per process)
    static int32_t* buf = nullptr;
    if (!buf) (void)hipMalloc(&buf, 16);
    kstat = buf;
    (void)hipMemsetAsync(kstat, 0, 16, st);
  }
#endif
#ifdef RPT_AB
  if (use_label_tiles())
    hipLaunchKernelGGL((k_label_tiles<false>), dim3(tile_grid_blocks()), dim3(kTileBlock), 0, st,
                       g, tile_R, tile_by, tile_nbands, (int64_t)g.nt * tile_nbands, occ,
                       n_occ_dev, rowq, rec<2>(), mutual, occ_bits, slab_t, pts, ccmin, cell_min,
                       sorig, mr, min_samples, labels);
  else if (cell_comp && ab().k7_w == 64)
    with_bool(bits, [&](auto b) {
      hipLaunchKernelGGL((k_label<2, false, 64, true, false, b.value>), dim3(wave_grid(n)),
                         dim3(kBlock), 0, st, pts, skey, g, rec<2>(), occ_bits, slab_t,
                         (const int32_t*)nullptr, cell_min, mutual, sorig, mr, nc_list, nc_count,
                         labels, (int32_t*)nullptr, core, core_bits);
    });
  else if (dim == 2 && ab().k7_w == 64)
    hipLaunchKernelGGL((k_label<2, false, 64>), dim3(wave_grid(n)), dim3(kBlock), 0, st, pts,
                       skey, g, rec<2>(), occ_bits, slab_t, ccmin, cell_min, mutual, sorig, mr,
                       nc_list, nc_count, labels);
  else
#endif
  if (cell_comp && xy_points)  // (xy_rule: integral eps_t windows, so bits)
    hipLaunchKernelGGL((k_label<2, false, 32, true, true, true>), dim3(wave_grid(n)),
                       dim3(kBlock), 0, st, reinterpret_cast<const Pt<true>*>(pts), skey, g,
                       rec<2>(), occ_bits, slab_t, (const int32_t*)nullptr, cell_min, mutual,
                       sorig, mr, nc_list, nc_count, labels, kstat, core, core_bits);
  else if (cell_comp)
    with_bool(bits, [&](auto b) {
      hipLaunchKernelGGL((k_label<2, false, 32, true, false, b.value>), dim3(wave_grid(n)),
                         dim3(kBlock), 0, st, pts, skey, g, rec<2>(), occ_bits, slab_t,
                         (const int32_t*)nullptr, cell_min, mutual, sorig, mr, nc_list, nc_count,
                         labels, kstat, core, core_bits);
    });
  else if (dim == 2)
    hipLaunchKernelGGL((k_label<2, false, 32>),
                       dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey, g,
                       rec<2>(), occ_bits, slab_t, ccmin, cell_min, mutual, sorig, mr, nc_list,
                       nc_count, labels, kstat);
  else
    hipLaunchKernelGGL((k_label<3, false, 64>),
                       dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey, g,
                       rec<3>(), occ_bits, slab_t, ccmin, cell_min, mutual, sorig, mr, nc_list,
                       nc_count, labels);
  RPT_CHECK_LAUNCH();
#ifdef RPT_AB
  if (kstat) {
    int32_t ks[4] = {0, 0, 0, 0};
    (void)hipMemcpyAsync(ks, kstat, 16, hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    std::fprintf(stderr,
                 "[rpt stats] n=%lld label: queued=%d core_in_window=%d searched=%d labelled=%d\n",
                 (long long)n, ks[0], ks[1], ks[2], ks[3]);
  }
#endif
  tm.mark();
  if (stats && defer) return RPT_OK;  // fill_stats after the caller's sync
  if (stats) {
    int32_t ncl = 0;
    RPT_HIP(hipMemcpyAsync(&ncl, n_clusters_ptr(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
    RPT_TRY(fill_stats(ncl, stats));
  }
  return RPT_OK;
}

int32_t DbscanState::fill_stats(int32_t ncl, rpt_stdbscan_stats* stats) {
  if (ncl < 0) {  // k_label_core_cells' guard
    set_error("rpt_stdbscan: a non-mutual cell on a grid taken for all-mutual (labels invalid)");
    return RPT_EHIP;
  }
  {
    stats->n_points = n;
    stats->n_clusters = ncl;
    stats->n_core = -1;
    stats->grid_dims[0] = g.nx;
    stats->grid_dims[1] = g.ny;
    stats->grid_dims[2] = g.nz;
    stats->grid_dims[3] = g.nt;
    stats->grid_cells = C;
    if (tm.on && tm.k >= 6) {
      RPT_HIP(hipEventSynchronize(tm.ev[tm.k - 1]));
      stats->ms_bounds = tm.ms(0);
      stats->ms_grid = tm.ms(1);
      stats->ms_core = tm.ms(2);
      stats->ms_union = tm.ms(3);
      stats->ms_label = tm.ms(4);
    }
  }
  return RPT_OK;
}

int32_t DbscanState::labels_global(const int64_t* rep_orig, const int64_t* reps, int64_t nr,
                                   int32_t* labels, hipStream_t st, const int64_t* nr_dev) {
  if (degenerate) {
    set_error("rpt_dbscan_labels_global: degenerate parameters are handled by rpt_stdbscan");
    return RPT_ENOTSUP;
  }
  RPT_TRY(need_float4("labels_global"));
  const int gb = grid_for(n, kBlock, 2048);
  int32_t* nc_count = nc_list + n;
  const bool cr = ab().cell_roots;
  if (cr) {  // (also clears nc_count for k_ccmin_global and fills cell_min with INT_MAX)
    hipLaunchKernelGGL(k_cell_roots, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st, parent,
                       occ, n_occ_dev, C, mutual, rep, cell_root, nc_count, (uint32_t*)nullptr,
                       (int64_t)0, cell_min);
  } else {
    RPT_HIP(hipMemsetAsync(nc_count, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(C, kBlock, 8192)), dim3(kBlock), 0, st, cell_min,
                       C, INT_MAX);
  }
  hipLaunchKernelGGL(k_ccmin_global, dim3(tile_grid(n)), dim3(kBlock), 0, st, parent, core, n,
                     sorig, rep_orig, reps, nr, ccmin, cid, nc_list, nc_count, skey, mutual,
                     cr ? (const int32_t*)cell_root : nullptr, C, nr_dev);
  // the core labels in original order (before slab's inverse permutation is overwritten), then
  // per sorted point the final core labels with the per-cell smallest label folded in
  // (k_cell_min_key's pass)
  const bool orig = spos_on;
  if (orig)
    hipLaunchKernelGGL(k_label_global_orig, dim3(grid_for(n, kBlock * kPU, 2048)), dim3(kBlock), 0,
                       st, core, ccmin, cid, slab, n, labels);
  hipLaunchKernelGGL(k_label_global_core, dim3(gb), dim3(kBlock), 0, st, core, ccmin, cid, sorig,
                     n, slab, orig ? nullptr : labels, skey, C, cell_min);
  // slab now holds the sorted points' core labels, no longer the inverse permutation: a second
  // call on this state (the shard driver's redo of a step whose pairs / results overflowed, a
  // host merge, the K9 radix fallback) takes the sorted-order path
  spos_on = false;
#ifdef RPT_AB
  if (use_label_tiles())
    hipLaunchKernelGGL((k_label_tiles<true>), dim3(tile_grid_blocks()), dim3(kTileBlock), 0, st,
                       g, tile_R, tile_by, tile_nbands, (int64_t)g.nt * tile_nbands, occ,
                       n_occ_dev, rowq, rec<2>(), mutual, occ_bits, slab_t, pts, slab, cell_min,
                       sorig, MinRank{nullptr, nullptr}, min_samples, labels);
  else if (dim == 2 && ab().k7_w == 64)
    hipLaunchKernelGGL((k_label<2, true, 64>), dim3(wave_grid(n)), dim3(kBlock), 0, st, pts,
                       skey, g, rec<2>(), occ_bits, slab_t, slab, cell_min, mutual, sorig,
                       MinRank{nullptr, nullptr}, nc_list, nc_count, labels);
  else
#endif
  with_dim(dim, [&](auto d) {  // (W: a point per half-wave in 2-D, per wave in 3-D)
    hipLaunchKernelGGL((k_label<d.value, true, d.value == 2 ? 32 : 64>), dim3(wave_grid(n)),
                       dim3(kBlock), 0, st, pts, skey, g, rec<d.value>(), occ_bits, slab_t, slab,
                       cell_min, mutual, sorig, MinRank{nullptr, nullptr}, nc_list, nc_count,
                       labels);
  });
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t DbscanState::frames_pass(int32_t min_frames, hipStream_t st) {
  if (degenerate || min_frames < 1) return RPT_OK;  // <= 0: every core point qualifies
  RPT_TRY(need_float4("frames_pass"));
  cmin_ready = false;  // core points may be demoted below
  const bool refine = min_frames >= 2;
  int32_t* list = nc_list;  // free until labels_fifo rebuilds it
  int32_t* count = nc_list + n;
  const int32_t* n_occ = n_occ_dev;
  const bool cells = refine && integral_t && dim == 2 && g.nz == 1;
  // a whole-cell hit is one frame only when a slab is one frame: the cell cap can widen the slabs
  // (ct = 2, 4, ... for long runs of frames over a small region), then every point is read
  const int one_frame_cells = (integral_t && g.ct == 1.0) ? 1 : 0;
  if (cells) {
    const int R = (int)std::min<double>(std::floor((double)g.epst / g.ct), 64.0);
    hipLaunchKernelGGL(k_frames_cells, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, st, g, R,
                       occ, n_occ, rec<2>(), occ_bits, min_frames, fok);
  }
  RPT_TRY(zero_n(st, 1, &count));
  hipLaunchKernelGGL(k_frames_queue, dim3(tile_grid(n)), dim3(kBlock), 0, st, skey, n, C,
                     cells ? (const uint8_t*)fok : (const uint8_t*)nullptr, (int)min_frames,
                     refine ? 1 : 0, core, list, count);
  if (refine) {
    // offsets of int32(t) within +-31 of the point's own frame fit the 64-bit set (|dt| <=
    // eps_t <= 30); larger windows list the distinct frames instead
    const bool small = (double)g.epst <= 30.0;
    if (small)
      with_dim(dim, [&](auto d) {
        hipLaunchKernelGGL(k_frames_points<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts,
                           skey, g, rec<d.value>(), occ_bits, slab_t, one_frame_cells,
                           (int)min_frames, list, count, core);
      });
    else
      with_dim(dim, [&](auto d) {
        hipLaunchKernelGGL(k_frames_points_list<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st,
                           pts, skey, g, rec<d.value>(), occ_bits, slab_t, one_frame_cells,
                           (int)min_frames, list, count, core);
      });
  }
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t DbscanState::labels_fifo(int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st) {
  RPT_TRY(need_float4("labels_fifo"));
  int32_t* nc_count = nc_list + n;  // k_ccmin's non-core queue counter, cleared by cluster_ids
  int32_t* spos = slab;
  RPT_TRY(cluster_ids(st, nullptr, nc_count));
  if (!spos_on)  // (else the grid build's)
    hipLaunchKernelGGL(k_inverse_perm, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st,
                       sorig, n, spos);
  const MinRank mr{min_bits, min_pref};
  hipLaunchKernelGGL(k_label_core_orig, dim3((grid_for(n, kBlock * kPU, 2048) + 7) & ~7),
                     dim3(kBlock), 0, st, ccmin, n, spos, mr, labels);
  with_dim(dim, [&](auto d) {
    hipLaunchKernelGGL(k_label_fifo<d.value>, dim3(wave_grid(n)), dim3(kBlock), 0, st, pts, skey,
                       g, rec<d.value>(), occ_bits, slab_t, ccmin, rep, sorig, spos, mr, nc_list,
                       nc_count, labels);
  });
  RPT_CHECK_LAUNCH();
  tm.mark();
  int32_t ncl = 0;
  RPT_HIP(hipMemcpyAsync(&ncl, n_clusters_ptr(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  if (stats) RPT_TRY(fill_stats(ncl, stats));
  return RPT_OK;
}

static int32_t check_args(const float* x, const float* y, const float* z, int64_t stride,
                          const float* t, int64_t n, int dim) {
  if (n <= 0) {
    set_error("Found array with 0 sample(s) (shape=(0, %d)) while a minimum of 1 is required.",
              dim);
    return RPT_EEMPTY;
  }
  if (n >= (int64_t(1) << 31) - 2) {
    set_error("rpt_stdbscan: n=%lld exceeds the int32 index space", (long long)n);
    return RPT_ENOTSUP;
  }
  if (!x || !y || !t || (dim == 3 && !z) || stride < 1) {
    set_error("rpt_stdbscan: null pointer or bad stride");
    return RPT_EINVAL;
  }
  return RPT_OK;
}

static std::mutex g_state_mu;
// per (device, stream), for the fused single-call path
static std::vector<std::pair<std::pair<int, hipStream_t>, DbscanState*>> g_states;
// *S: the state of (the current device, st), created at its first use
static int32_t state_for(hipStream_t st, DbscanState** S) {
  int dev = 0;
  RPT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_state_mu);
  *S = nullptr;
  for (auto& e : g_states)
    if (e.first.first == dev && e.first.second == st) *S = e.second;
  if (!*S) {
    *S = new DbscanState();
    g_states.push_back({{dev, st}, *S});
  }
  return RPT_OK;
}

int32_t stdbscan(const float* x, const float* y, const float* z, int64_t stride, const float* t,
                 int64_t n, double eps_space, double eps_time, int32_t min_samples,
                 int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st, int dim) {
  RPT_TRY(check_args(x, y, z, stride, t, n, dim));
  if (!labels) {
    set_error("rpt_stdbscan: null labels");
    return RPT_EINVAL;
  }
  DbscanState* S;
  RPT_TRY(state_for(st, &S));
  S->may_xy = stats != nullptr;  // (with stats: union_pass runs fused)
  RPT_TRY(S->build(x, y, z, stride, t, n, eps_space, eps_time, min_samples,
                   stats && stats->timing, st));
  RPT_TRY(S->core_pass(st));
  RPT_TRY(S->union_pass(st, stats != nullptr));  // (the guard needs labels_local's readback)
  return S->labels_local(labels, stats, st);
}

// the state's sorted counts in original order (zeros for degenerate parameters: no pair passes)
static int32_t counts_out(DbscanState* S, int32_t* counts, hipStream_t st) {
  if (S->degenerate) {
    RPT_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)S->n, st));
    return RPT_OK;
  }
  hipLaunchKernelGGL(k_counts_to_orig, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                     S->counts, S->sorig, S->n, counts);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t neighbour_counts(const float* x, const float* y, const float* z, int64_t stride,
                         const float* t, int64_t n, double eps_space, double eps_time,
                         int32_t* counts, hipStream_t st, int dim) {
  if (n < 0) {
    set_error("rpt_neighbour_counts: n < 0");
    return RPT_EINVAL;
  }
  RPT_TRY(check_args(x, y, z, stride, t, n, dim));
  if (!counts) {
    set_error("rpt_neighbour_counts: null counts");
    return RPT_EINVAL;
  }
  DbscanState* S;
  RPT_TRY(state_for(st, &S));
  // (min_samples 1: the grid build reads only its sign)
  RPT_TRY(S->build(x, y, z, stride, t, n, eps_space, eps_time, 1, false, st));
  RPT_TRY(S->count_pass(S->counts, st));
  return counts_out(S, counts, st);
}

int32_t stdbscan_sweep(const float* x, const float* y, const float* z, int64_t stride,
                       const float* t, int64_t n, double eps_space, double eps_time,
                       const int32_t* min_samples, int32_t n_sets, int32_t* counts,
                       int32_t* labels, rpt_stdbscan_stats* stats, hipStream_t st, int dim) {
  if (n < 0) {
    set_error("rpt_stdbscan_sweep: n < 0");
    return RPT_EINVAL;
  }
  if (!min_samples || n_sets < 1 || n_sets > 64) {
    set_error("rpt_stdbscan_sweep: n_sets must be 1 .. 64 and min_samples non-null");
    return RPT_EINVAL;
  }
  for (int32_t k = 0; k < n_sets; ++k)
    if (min_samples[k] < 1) {
      set_error("rpt_stdbscan_sweep: min_samples[%d] = %d, every entry must be >= 1", (int)k,
                (int)min_samples[k]);
      return RPT_EINVAL;
    }
  RPT_TRY(check_args(x, y, z, stride, t, n, dim));
  if (!labels) {
    set_error("rpt_stdbscan_sweep: null labels");
    return RPT_EINVAL;
  }
  DbscanState* S;
  RPT_TRY(state_for(st, &S));
  S->defer = false;  // every set's labels_local reads its cluster count back
  const bool timing = stats && stats[0].timing;
  RPT_TRY(S->build(x, y, z, stride, t, n, eps_space, eps_time, min_samples[0], timing, st));
  RPT_TRY(S->count_pass(S->counts, st));  // (the timer's "core" interval)
  if (counts) RPT_TRY(counts_out(S, counts, st));
  for (int32_t k = 0; k < n_sets; ++k) {
    rpt_stdbscan_stats* sk = stats ? stats + k : nullptr;
    if (k > 0 && S->tm.on) {  // this set's union / label intervals over the first set's events
      S->tm.k = 3;
      S->tm.mark();
    }
    RPT_TRY(S->core_from_counts(S->counts, min_samples[k], st));
    int32_t n_core = 0;
    if (sk && !S->degenerate)  // (read by labels_local's synchronisation below)
      RPT_HIP(hipMemcpyAsync(&n_core, S->n_core_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RPT_TRY(S->union_pass(st, sk != nullptr));  // (the guard needs labels_local's readback)
    RPT_TRY(S->labels_local(labels + (size_t)k * (size_t)n, sk, st));
    if (sk) {
      sk->n_core = n_core;
      if (k > 0) sk->ms_bounds = sk->ms_grid = sk->ms_core = 0.0;
    }
  }
  return RPT_OK;
}

// Denoise variant (PointCloudWorkF/stdbscan_denoising_pipeline.py:264-369), 2-D.
int32_t stdbscan_denoise(const float* x, const float* y, const float* t, int64_t n,
                         double eps_space, double eps_time, int32_t min_samples,
                         int32_t min_frames, int32_t* labels, rpt_stdbscan_stats* stats,
                         hipStream_t st) {
  if (n == 0) {  // the reference returns an empty label array (:286-287), no error
    if (stats) *stats = rpt_stdbscan_stats{};
    return RPT_OK;
  }
  RPT_TRY(check_args(x, y, nullptr, 1, t, n, 2));
  if (!labels) {
    set_error("rpt_stdbscan_denoise: null labels");
    return RPT_EINVAL;
  }
  if (min_frames > 64 * kFramesPerLane && !((float)eps_time <= 30.0f) &&
      (float)eps_time == (float)eps_time) {
    set_error("rpt_stdbscan_denoise: min_frames > %d with eps_time > 30 is not supported",
              64 * kFramesPerLane);
    return RPT_ENOTSUP;
  }
  DbscanState* S;
  RPT_TRY(state_for(st, &S));
  RPT_TRY(S->build(x, y, nullptr, 1, t, n, eps_space, eps_time, min_samples,
                   stats && stats->timing, st));
  if (S->degenerate) {
    // no pair passes (not even (i, i)): core iff 0 >= min_samples and 0 >= min_frames, each its
    // own cluster in index order
    const bool single = min_samples <= 0 && min_frames <= 0;
    hipLaunchKernelGGL(k_isolated_labels, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st,
                       labels, n, single ? 1 : 0);
    RPT_CHECK_LAUNCH();
    if (stats) {
      stats->n_points = n;
      stats->n_core = single ? n : 0;
      stats->n_clusters = single ? (int32_t)n : 0;
    }
    return wait_stream(st);
  }
  RPT_TRY(S->core_pass(st));
  RPT_TRY(S->frames_pass(min_frames, st));
  RPT_TRY(S->union_pass(st));
  return S->labels_fifo(labels, stats, st);
}

// ---- the bounds passes and the deferred form (the native stack driver; stdbscan.h)
size_t stdbscan_bounds_bytes() { return sizeof(Bounds); }
int32_t stdbscan_bounds_dev(const float* x, const float* y, const float* t, int64_t n_max,
                            const int64_t* n_dev, void* out_dev, void* part_dev,
                            hipStream_t st) {
  const int nbb = grid_for(std::max<int64_t>(n_max, 1), kBlock, 1024);
  hipLaunchKernelGGL(k_bounds<2>, dim3(nbb), dim3(kBlock), 0, st, x, y, (const float*)nullptr,
                     (int64_t)1, t, n_max, static_cast<Bounds*>(part_dev), n_dev);
  hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(kBlock), 0, st,
                     static_cast<const Bounds*>(part_dev), nbb, static_cast<Bounds*>(out_dev));
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
int32_t stdbscan_bounds_final_dev(const void* part_dev, int nb, void* out_dev, hipStream_t st) {
  hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(kBlock), 0, st,
                     static_cast<const Bounds*>(part_dev), nb, static_cast<Bounds*>(out_dev));
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
static_assert(kBlock == kBoundsBlock, "k_bounds is launched with kBlock threads per block");
size_t stdbscan_bounds_part_bytes(int64_t n_max) {
  return sizeof(Bounds) * (size_t)grid_for(std::max<int64_t>(n_max, 1), kBoundsBlock, 1024);
}

int32_t stdbscan_deferred(const float* x, const float* y, const float* z, int64_t stride,
                          const float* t, int64_t n, double eps_space, double eps_time,
                          int32_t min_samples, int32_t* labels, rpt_stdbscan_stats* stats,
                          hipStream_t st, int dim, const int32_t** n_clusters_dev,
                          void** state, const void* host_bounds) {
  RPT_TRY(check_args(x, y, z, stride, t, n, dim));
  if (!labels || !stats || !n_clusters_dev || !state) {
    set_error("stdbscan_deferred: null argument");
    return RPT_EINVAL;
  }
  DbscanState* S;
  RPT_TRY(state_for(st, &S));
  S->given_bounds = host_bounds;
  S->may_xy = true;
  const int32_t sb = S->build(x, y, z, stride, t, n, eps_space, eps_time, min_samples,
                              stats->timing != 0, st);
  S->given_bounds = nullptr;
  RPT_TRY(sb);
  RPT_TRY(S->core_pass(st));
  RPT_TRY(S->union_pass(st, true));
  S->defer = !S->degenerate;
  const int32_t s_ = S->labels_local(labels, stats, st);
  *n_clusters_dev = S->defer ? S->n_clusters_ptr() : nullptr;
  *state = S;
  return s_;
}

int32_t stdbscan_core_flags(void* state, int64_t n, uint8_t* out, hipStream_t st) {
  DbscanState* S = static_cast<DbscanState*>(state);
  if (!S || S->degenerate || S->n != n || !S->core || !S->sorig) {
    set_error("rpt_stack_core_flags: no core flags for this run");
    return RPT_EINVAL;
  }
  hipLaunchKernelGGL(k_core_to_orig, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, st,
                     S->core, S->sorig, n, out);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t stdbscan_fill_stats(void* state, int32_t n_clusters, rpt_stdbscan_stats* stats) {
  DbscanState* S = static_cast<DbscanState*>(state);
  S->defer = false;
  return S->fill_stats(n_clusters, stats);
}

// ---- phased C-ABI bodies
DbscanState* dbscan_create() { return new DbscanState(); }
void dbscan_destroy(DbscanState* s) {
  if (s) {
    s->arena.release();
    delete s;
  }
}
int32_t dbscan_build(DbscanState* S, const float* x, const float* y, const float* z,
                     int64_t stride, const float* t, int64_t n, double eps_space,
                     double eps_time, int32_t ms, hipStream_t st) {
  RPT_TRY(check_args(x, y, z, stride, t, n, z ? 3 : 2));
  RPT_TRY(S->build(x, y, z, stride, t, n, eps_space, eps_time, ms, false, st));
  if (S->degenerate) {
    set_error("rpt_dbscan_build: negative or NaN eps (use rpt_stdbscan)");
    return RPT_ENOTSUP;
  }
  return RPT_OK;
}
int32_t dbscan_core(DbscanState* S, uint8_t* core_out, hipStream_t st) {
  RPT_TRY(S->core_pass(st));
  if (core_out) {
    hipLaunchKernelGGL(k_core_to_orig, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                       S->core, S->sorig, S->n, core_out);
    RPT_CHECK_LAUNCH();
  }
  return RPT_OK;
}
int32_t dbscan_set_core(DbscanState* S, const uint8_t* core_in, hipStream_t st) {
  S->cmin_ready = false;
  hipLaunchKernelGGL(k_core_from_orig, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                     core_in, S->sorig, S->n, S->core);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
int32_t dbscan_components(DbscanState* S, int32_t* comp_out, hipStream_t st) {
  RPT_TRY(S->union_pass(st));
  if (S->degenerate || S->n == 0) {  // (no cell structure: every core point walks its chain)
    hipLaunchKernelGGL(k_comp_out, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                       S->parent, S->core, S->sorig, S->n, comp_out, S->skey,
                       (const int32_t*)nullptr, (int64_t)0);
  } else {
    hipLaunchKernelGGL(k_cell_roots, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                       S->parent, S->occ, S->n_occ_dev, S->C, S->mutual, S->rep, S->cell_root,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(k_comp_out, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                       S->parent, S->core, S->sorig, S->n, comp_out, S->skey,
                       (const int32_t*)S->cell_root, S->C);
  }
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
int32_t dbscan_components_edges(DbscanState* S, int32_t* comp_out, int64_t lo_end,
                                int64_t hi_begin, hipStream_t st) {
  if (lo_end >= hi_begin) return dbscan_components(S, comp_out, st);
  RPT_TRY(S->union_pass(st));
  if (S->n == 0) return RPT_OK;
  const bool cells = !S->degenerate;
  if (cells)
    hipLaunchKernelGGL(k_cell_roots, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                       S->parent, S->occ, S->n_occ_dev, S->C, S->mutual, S->rep, S->cell_root,
                       (int32_t*)nullptr);
  hipLaunchKernelGGL(k_comp_out_edges, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                     S->parent, S->core, S->sorig, S->n, comp_out, S->skey,
                     cells ? (const int32_t*)S->cell_root : nullptr, cells ? S->C : (int64_t)0,
                     lo_end, hi_begin);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
void dbscan_uf_arrays(const DbscanState* S, const uint8_t** core, const int32_t** parent,
                      const int32_t** sorig, int64_t* n) {
  *core = S->core;
  *parent = S->parent;
  *sorig = S->sorig;
  *n = S->n;
}
int32_t dbscan_labels_global(DbscanState* S, const int64_t* rep, const int64_t* reps, int64_t nr,
                             int32_t* labels, hipStream_t st) {
  return S->labels_global(rep, reps, nr, labels, st);
}
// ---- the frame-sharded driver's forms (stdbscan.h)
int32_t dbscan_build_given(DbscanState* S, const float* x, const float* y, const float* t,
                           int64_t n, double eps_space, double eps_time, int32_t ms,
                           const void* host_bounds, hipStream_t st) {
  RPT_TRY(check_args(x, y, nullptr, 1, t, n, 2));
  S->given_bounds = host_bounds;
  const int32_t s_ = S->build(x, y, nullptr, 1, t, n, eps_space, eps_time, ms, false, st);
  S->given_bounds = nullptr;
  RPT_TRY(s_);
  if (S->degenerate) {
    set_error("rpt_shard: negative or NaN eps");
    return RPT_ENOTSUP;
  }
  return RPT_OK;
}
int32_t dbscan_labels_global_dev(DbscanState* S, const int64_t* rep, const int64_t* reps,
                                 const int64_t* nr_dev, int32_t* labels, hipStream_t st) {
  return S->labels_global(rep, reps, 0, labels, st, nr_dev);
}
// the kernels of dbscan_core_edges / dbscan_set_core_edges: one pass over the sorted points
__global__ void k_core_to_orig_ranges(const uint8_t* __restrict__ core,
                                      const int32_t* __restrict__ sorig, int64_t n, int64_t a0,
                                      int64_t a1, uint8_t* __restrict__ out_a, int64_t b0,
                                      int64_t b1, uint8_t* __restrict__ out_b) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = sorig[s];
    if (out_a && i >= a0 && i < a1) out_a[i - a0] = core[s];
    if (out_b && i >= b0 && i < b1) out_b[i - b0] = core[s];
  }
}
__global__ void k_core_from_orig_ranges(const uint8_t* __restrict__ in_a, int64_t a1,
                                        const uint8_t* __restrict__ in_b, int64_t b0,
                                        const int32_t* __restrict__ sorig, int64_t n,
                                        uint8_t* __restrict__ core) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = sorig[s];
    if (in_a && i < a1) core[s] = in_a[i];
    if (in_b && i >= b0) core[s] = in_b[i - b0];
  }
}
int32_t dbscan_core_edges(DbscanState* S, int64_t a0, int64_t a1, uint8_t* out_a, int64_t b0,
                          int64_t b1, uint8_t* out_b, hipStream_t st) {
  if (S->n <= 0 || (!(out_a && a1 > a0) && !(out_b && b1 > b0))) return RPT_OK;
  hipLaunchKernelGGL(k_core_to_orig_ranges, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0,
                     st, S->core, S->sorig, S->n, a0, a1, a1 > a0 ? out_a : nullptr, b0, b1,
                     b1 > b0 ? out_b : nullptr);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
int32_t dbscan_set_core_edges(DbscanState* S, const uint8_t* in_a, int64_t a1,
                              const uint8_t* in_b, int64_t b0, hipStream_t st) {
  const bool a = in_a && a1 > 0, b = in_b && b0 < S->n;
  if (S->n <= 0 || (!a && !b)) return RPT_OK;
  S->cmin_ready = false;  // core flags change: the core pass's cell minima no longer hold
  hipLaunchKernelGGL(k_core_from_orig_ranges, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0,
                     st, a ? in_a : nullptr, a1, b ? in_b : nullptr, b0, S->sorig, S->n, S->core);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
int32_t dbscan_core_orig(DbscanState* S, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(k_core_to_orig, dim3(grid_for(S->n, kBlock, 2048)), dim3(kBlock), 0, st,
                     S->core, S->sorig, S->n, out);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

}  // namespace rpt
