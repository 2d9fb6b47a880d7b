// ST-DBSCAN, what more than one stage file or the DbscanState driver reads; no kernel is here.
// In order: kBlock, the order-preserving float key (f2ord) and the DPP row reductions;
// the grid geometry (FastDiv, Geom, cell_of, slab_of) and the sorted-point layouts (PtRec,
// Pt<XY>, load_pt, store_pt, slab_time_of); occupied, the launch grids of the persistent kernels
// (wave_grid, tile_grid), the wave reductions and the cell record (CellRec<D>, rec_boxA /
// rec_boxB); the neighbour predicates, for_each_cell, rep_id, the block-aggregated append, the
// candidate windows, classify_cells and the XCD item split (XcdRange, xcd_items);
// write_cell_flags (K5's cell kernels and the A/B-only forms); last the constants that two
// stages share: kR and kPmaskFull (K5's window scans and K6's candidate masks), kCwMaxR (K5's
// eight-lane kernels and DbscanState::oct_ok) and kPU (K6's star initialisation, the label
// kernels and the driver's grids for both).
// The union-find helpers (uf_*, BlockList, block_last_wave, union_point) are not here: they stay
// with K6 in stdbscan_union.inc, and the files that read them from there say so.

constexpr int kBlock = 256;

// ---------------------------------------------------------------- order-preserving f32 <-> u32
__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// (ord2f, the host's way back: common.h)

// ---------------------------------------------------------------- cross-lane reductions by DPP
// __shfl_xor compiles to a ds_bpermute round trip through LDS, each one waited for; DPP moves
// are VALU.  Within an aligned row of 16 lanes, step k of row_reduce makes every lane of the
// aligned 2^k-lane group hold the group's result: lane i reads i^1, i^2 (quad permutes), then
// 7-i of its eight (row_half_mirror), then 15-i of its row (row_mirror).  Every lane of a group
// must be active.
template <int Ctl>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(0, v, Ctl, 0xF, 0xF, false);
}
template <int Ctl>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(dpp_mov<Ctl>(__float_as_int(v)));
}
template <int Ctl>
__device__ __forceinline__ uint64_t dpp_mov(uint64_t v) {
  const uint32_t lo = (uint32_t)dpp_mov<Ctl>((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)dpp_mov<Ctl>((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
template <int G, class T, class F>
__device__ __forceinline__ T row_reduce(T v, F op) {
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "groups within a row");
#ifdef RPT_DEBUG_DPP
  // (debug builds, -DRPT_DEBUG_DPP) the DPP moves read 0 from an inactive lane: a min would
  // return 0 and a sum drop terms, so every lane of this lane's aligned G-lane group must be
  // active -- all callers keep their loops group-uniform
  {
    const uint64_t act = __ballot(1);
    const int g0 = (int)(threadIdx.x & 63) & ~(G - 1);
    const uint64_t need = (G == 64 ? ~0ull : ((1ull << G) - 1)) << g0;
    if ((act & need) != need) __builtin_trap();
  }
#endif
  v = op(v, dpp_mov<0xB1>(v));                 // quad_perm [1,0,3,2]
  if (G >= 4) v = op(v, dpp_mov<0x4E>(v));     // quad_perm [2,3,0,1]
  if (G >= 8) v = op(v, dpp_mov<0x141>(v));    // row_half_mirror
  if (G >= 16) v = op(v, dpp_mov<0x140>(v));   // row_mirror
  return v;
}
struct OpMin {  // floats: fminf (the ignore-NaN minimum the shuffle form used)
  template <class T>
  __device__ T operator()(T a, T b) const { return b < a ? b : a; }
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct OpMax {
  template <class T>
  __device__ T operator()(T a, T b) const { return a < b ? b : a; }
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct OpAdd {
  template <class T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpOr {
  template <class T>
  __device__ T operator()(T a, T b) const { return a | b; }
};


// ---------------------------------------------------------------- grid geometry
// n / d for 0 <= n < 2^31 by one 32 x 32 -> 64-bit multiply and a shift (Granlund-Montgomery):
// m = ceil(2^(31+k) / d) with 2^(k-1) < d <= 2^k, so m < 2^32 and the rounding error n * (m / 2^(31+k)
// - 1 / d) < 2^-k <= 1 / d never reaches the next integer.  The cell-key decodes of the latency-
// bound window kernels divided by runtime grid sizes (a few dozen VALU instructions each).
struct FastDiv {
  uint32_t m;
  int s;
  void init(uint32_t d) {
    int k = 0;
    while ((uint64_t(1) << k) < d) ++k;
    s = 31 + k;
    m = (uint32_t)(((uint64_t(1) << s) + d - 1) / d);
  }
  __device__ __forceinline__ uint32_t div(uint32_t n) const {
    return (uint32_t)(((uint64_t)n * m) >> s);
  }
};

struct Geom {
  double ox, oy, oz, ot;  // origins (minima)
  double cs;              // spatial cell side
  double ct;              // time slab width
  double inv_cs, inv_ct;  // their float64 reciprocals (cell_of)
  int nx, ny, nz, nt;
  int64_t cells;          // nx*ny*nz*nt (an extra "isolated" cell C holds non-finite t)
  double eps2;            // eps_space^2 (float64)
  float epst;             // float32(eps_time)
  int min_samples;
  // float32 box-bound screen (classify_cells<D, true>): a float32 squared box distance <= e2lo
  // (> e2hi) is <= (>) eps2 in the float64 bound too (margins 1e-5 >> the float32 rounding);
  // e2lo = -1 / e2hi = inf disable it (eps2 outside [1e-20, 1e30])
  float e2lo, e2hi;
  // integral times (slabs hold whole time values): every neighbour of a point or cell in slab s
  // lies in slabs [s - rt, s + rt] (DbscanState::slab_reach), so the scan windows take exactly
  // those; -1: non-integral times, windows from the time range with one slab of slack each side
  int rt;
  // 1: every time is an integer and a slab is ONE time value (ct == 1), so any two points whose
  // slabs lie within rt <= floor(eps_t) of each other pass the time test: the window kernels, whose
  // candidates all come from such windows, skip the time bounds of their box classifications
  int tfree;
  FastDiv fnx, fny, fnz, fslab;  // by nx, ny, nz and nx * ny * nz (a key's slab)
  // cell key (< 2^31) -> x, y, z, slab
  __device__ __forceinline__ void split(uint32_t k, int& x, int& y, int& z, int& s) const {
    const uint32_t r = fnx.div(k);
    x = (int)(k - r * (uint32_t)nx);
    const uint32_t r2 = fny.div(r);
    y = (int)(r - r2 * (uint32_t)ny);
    if (nz == 1) {
      z = 0;
      s = (int)r2;
    } else {
      const uint32_t r3 = fnz.div(r2);
      z = (int)(r2 - r3 * (uint32_t)nz);
      s = (int)r3;
    }
  }
  __device__ __forceinline__ int slab_of_key(int64_t k) const { return (int)fslab.div((uint32_t)k); }
};

// cell index floor((v - o) / side) as a multiply by the host's float64 reciprocal (a float64
// divide per coordinate dominated the grid build); every kernel assigns cells through this one
// function, so assignments stay consistent, and the 2^-20 margin on the side keeps every
// neighbour within +-2 cells whatever the last-bit rounding
__device__ __forceinline__ int cell_of(double v, double o, double inv, int n) {
  double q = floor((v - o) * inv);
  int c = (q < 0.0) ? 0 : (q >= (double)n ? n - 1 : (int)q);
  return c;
}
__device__ __forceinline__ int slab_of(float t, const Geom& g) {
  return cell_of((double)t, g.ot, g.inv_ct, g.nt);
}

// A sorted point: float4 {x, y, z|t, t}, or float2 {x, y} where no kernel of the run needs a
// point's time (XY; DbscanState::xy_points: Geom::tfree windows, one time value per slab, which
// the cell records and slab_t carry).  load_pt's z / w are NaN in xy form: a time test that
// reached them would pass for no pair.
template <bool XY>
struct PtRec {
  using type = float4;
};
template <>
struct PtRec<true> {
  using type = float2;
};
template <bool XY>
using Pt = typename PtRec<XY>::type;
template <bool XY>
__device__ __forceinline__ float4 load_pt(const Pt<XY>* __restrict__ pts, int64_t i) {
  if constexpr (XY) {
    const float2 v = pts[i];
    return make_float4(v.x, v.y, NAN, NAN);
  } else {
    return pts[i];
  }
}
template <bool XY>
__device__ __forceinline__ void store_pt(Pt<XY>* __restrict__ pts, int64_t i, float x, float y,
                                         float t) {
  if constexpr (XY)
    pts[i] = make_float2(x, y);
  else
    pts[i] = make_float4(x, y, t, t);
}
// xy form: the writer's own per-slab time range (what k_slab_range derives from the cell records
// otherwise): the slab's one time value read from its first point, (FLT_MAX, -FLT_MAX) when empty
__device__ __forceinline__ float2 slab_time_of(const float* __restrict__ t, int lo, int hi) {
  if (lo >= hi) return make_float2(FLT_MAX, -FLT_MAX);
  const float v = t[lo];
  return make_float2(v, v);
}

__device__ __forceinline__ bool occupied(const uint32_t* __restrict__ bits, int64_t c) {
  return (bits[c >> 5] >> (c & 31)) & 1u;
}

// grids of the persistent wave-per-item kernels (item counts live on the device)
inline int wave_grid(int64_t max_items) {  // a multiple of 8 blocks (XCD-aware ranges)
  const int g = grid_for(max_items, kBlock / 64, ab().wave_grid_cap);
  return (g + 7) & ~7;
}
inline int tile_grid(int64_t n) { return grid_for(n, kBlock * 16, 2048); }

__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// whole-wave sum (every lane active): rows by DPP, then the four row sums read as scalars
__device__ __forceinline__ int wave_sum(int v) {
  v = row_reduce<16>(v, OpAdd{});
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
         __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ int wave_excl_sum(int v, int* total) {
  const int lane = threadIdx.x & 63;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}
__device__ __forceinline__ int64_t wave_min64(int64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

// Per occupied cell, its point range and bounding box in ONE record (32 B in 2-D, 48 B in 3-D), so
// a candidate cell of a window scan costs one load; empty cells are zero (b == e).
template <int D>
struct CellRec;
template <>
struct alignas(16) CellRec<2> {
  int b, e;
  float x0, x1, y0, y1, t0, t1;
};
template <>
struct alignas(16) CellRec<3> {
  int b, e;
  float x0, x1, y0, y1, z0, z1, t0, t1;
  int pad0, pad1;
};
template <int D>
__device__ __forceinline__ float4 rec_boxA(const CellRec<D>& r) {
  return make_float4(r.x0, r.x1, r.y0, r.y1);
}
__device__ __forceinline__ float4 rec_boxB(const CellRec<2>& r) {
  return make_float4(r.t0, r.t1, r.t0, r.t1);
}
__device__ __forceinline__ float4 rec_boxB(const CellRec<3>& r) {
  return make_float4(r.z0, r.z1, r.t0, r.t1);
}

// ---------------------------------------------------------------- neighbour predicates

// Exact pair test (see file header): the float64 squared distance against eps^2.  A float32
// screen decides first (Geom::e2lo / e2hi, the classify_cells screen): the float32 distance is
// within a few 2^-24 of the float64 one (relative), far inside the 1e-5 margins, so only pairs
// within 1e-5 of eps reach the float64 test -- the float64 ops (half rate, plus conversions) were
// most of the VALU of the pair-testing kernels.
// XY (points loaded from the float2 layout: Geom::tfree windows, every pair within eps_t): x and
// y only.
template <int D, bool XY = false>
__device__ __forceinline__ bool adjacent(const float4& a, const float4& b, const Geom& g) {
  const float dt = XY ? 0.f : fabsf(a.w - b.w);
  const float fx = a.x - b.x, fy = a.y - b.y;
  float f2 = fx * fx + fy * fy;
  if (D == 3) {
    const float fz = a.z - b.z;
    f2 = f2 + fz * fz;
  }
  bool near = !(f2 <= g.e2lo) && !(f2 > g.e2hi);  // (NaN: near, the float64 test decides)
  bool in = f2 <= g.e2lo;
  if (near) {
    const double dx = (double)a.x - (double)b.x;
    const double dy = (double)a.y - (double)b.y;
    double d2 = dx * dx + dy * dy;
    if (D == 3) {
      const double dz = (double)a.z - (double)b.z;
      d2 = d2 + dz * dz;
    }
    in = d2 <= g.eps2;
  }
  return XY ? in : (in && (dt <= g.epst));
}

// |p - [lo, hi]| lower bound and the farthest-end distance, float64, each rounded like the pair
// test (monotone), so classification never contradicts the pair test.
__device__ __forceinline__ void span_dist(float p, float lo, float hi, double& dmin,
                                          double& dmax) {
  const double dp = (double)p;
  dmin = (p < lo) ? ((double)lo - dp) : ((p > hi) ? (dp - (double)hi) : 0.0);
  dmax = fmax(fabs(dp - (double)lo), fabs(dp - (double)hi));
}

// 0: no point of the cell can be adjacent; 1: every point is adjacent; 2: test pairs.
// XY: as adjacent<D, true>, no time bounds (the cell comes from the point's tfree window).
template <int D, bool XY = false>
__device__ __forceinline__ int classify(const float4& p, const float4& A, const float4& B,
                                        const Geom& g) {
  // time (float32, same rounding as the pair test)
  float tmax = 0.f;
  if constexpr (!XY) {
    const float tlo = B.z, thi = B.w;
    const float tmin = (p.w < tlo) ? (tlo - p.w) : ((p.w > thi) ? (p.w - thi) : 0.f);
    if (!(tmin <= g.epst)) return 0;
    tmax = fmaxf(fabsf(p.w - tlo), fabsf(p.w - thi));
  }
  {
    // float32 screen of the spatial bounds (as adjacent / classify_cells): float64 only when a
    // bound lies within 1e-5 of eps^2
    auto fgap = [](float v, float lo, float hi) { return fmaxf(fmaxf(lo - v, v - hi), 0.f); };
    auto fspan = [](float v, float lo, float hi) { return fmaxf(fabsf(v - lo), fabsf(v - hi)); };
    const float gx = fgap(p.x, A.x, A.y), gy = fgap(p.y, A.z, A.w);
    const float sx = fspan(p.x, A.x, A.y), sy = fspan(p.y, A.z, A.w);
    float fmn = gx * gx + gy * gy, fmx = sx * sx + sy * sy;
    if (D == 3) {
      const float gz = fgap(p.z, B.x, B.y), sz = fspan(p.z, B.x, B.y);
      fmn = fmn + gz * gz;
      fmx = fmx + sz * sz;
    }
    if (fmn > g.e2hi) return 0;
    if (fmx <= g.e2lo) return (tmax <= g.epst) ? 1 : 2;
    if (fmn <= g.e2lo && fmx > g.e2hi) return 2;
  }
  double mnx, mxx, mny, mxy;
  span_dist(p.x, A.x, A.y, mnx, mxx);
  span_dist(p.y, A.z, A.w, mny, mxy);
  double dmin = mnx * mnx + mny * mny;
  double dmax = mxx * mxx + mxy * mxy;
  if (D == 3) {
    double mnz, mxz;
    span_dist(p.z, B.x, B.y, mnz, mxz);
    dmin = dmin + mnz * mnz;
    dmax = dmax + mxz * mxz;
  }
  if (!(dmin <= g.eps2)) return 0;
  return (dmax <= g.eps2 && tmax <= g.epst) ? 1 : 2;
}

// Candidate-cell enumeration shared by the three scan kernels.  Calls f(cell, begin, end, cls)
// for every non-empty cell that may hold a neighbour of point p (own cell included); f returns
// true to stop the enumeration.
template <int D, class F>
__device__ __forceinline__ void for_each_cell(const float4& p, int32_t key, const Geom& g,
                                              const int32_t* __restrict__ cell_start,
                                              const CellRec<D>* __restrict__ crec,
                                              const float2* __restrict__ slab_t, F&& f) {
  int cx, cy, cz, cs;
  g.split((uint32_t)key, cx, cy, cz, cs);
  // conservative slab window (+-1 slack), culled by each slab's actual time range
  const double tp = (double)p.w, et = (double)g.epst;
  int s0 = (int)fmax(floor((tp - et - g.ot) * g.inv_ct) - 1.0, 0.0);
  int s1 = (int)fmin(floor((tp + et - g.ot) * g.inv_ct) + 1.0, (double)(g.nt - 1));
  const int x0 = max(cx - 2, 0), x1 = min(cx + 2, g.nx - 1);
  const int y0 = max(cy - 2, 0), y1 = min(cy + 2, g.ny - 1);
  const int z0 = (D == 3) ? max(cz - 2, 0) : 0, z1 = (D == 3) ? min(cz + 2, g.nz - 1) : 0;
  (void)cs;
  for (int s = s0; s <= s1; ++s) {
    const float2 sr = slab_t[s];
    if (sr.x > sr.y) continue;  // empty slab
    const float smin = (p.w < sr.x) ? (sr.x - p.w) : ((p.w > sr.y) ? (p.w - sr.y) : 0.f);
    if (!(smin <= g.epst)) continue;
    for (int zz = z0; zz <= z1; ++zz) {
      for (int yy = y0; yy <= y1; ++yy) {
        const int64_t row = (((int64_t)s * g.nz + zz) * g.ny + yy) * g.nx;
        int b = cell_start[row + x0];
        for (int xx = x0; xx <= x1; ++xx) {
          const int e = cell_start[row + xx + 1];
          if (e > b) {
            const int64_t c = row + xx;
            const CellRec<D> cr = crec[c];
            const int cls = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
            if (cls != 0 && f(c, b, e, cls)) return;
          }
          b = e;
        }
      }
    }
  }
}

__device__ __forceinline__ int32_t rep_id(const int64_t* __restrict__ reps, int64_t nr, int64_t v) {
  int64_t lo = 0, hi = nr;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (reps[m] < v) lo = m + 1; else hi = m;
  }
  return (lo < nr && reps[lo] == v) ? (int32_t)lo : -2;  // -2: representative missing (bug)
}

// ---------------------------------------------------------------- block-aggregated append
// Every thread of the block evaluates pred(s) for kItems sorted indices of one 256*kItems tile;
// the indices with pred true are appended to list with ONE global atomic per tile (thousands of
// same-address atomics per launch otherwise serialise in L2).  Order inside a tile is
// thread-major; consumers do not depend on the order.
constexpr int kItems = 16;
struct AppendIndex {
  __device__ int32_t operator()(int64_t s) const { return (int32_t)s; }
};
// Same, with this thread's predicate bits already known (bit k <-> index tile0 + k*kBlock + tid).
template <class V = AppendIndex>
__device__ __forceinline__ void block_append_bits(int64_t tile0, uint32_t bits,
                                                  int32_t* __restrict__ list,
                                                  int32_t* __restrict__ counter, V value = V{});

template <class P, class V = AppendIndex>
__device__ __forceinline__ void block_append(int64_t tile0, int64_t n, P&& pred,
                                             int32_t* __restrict__ list,
                                             int32_t* __restrict__ counter, V value = V{}) {
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t s = tile0 + (int64_t)k * kBlock + threadIdx.x;
    if (s < n && pred(s)) bits |= 1u << k;
  }
  block_append_bits(tile0, bits, list, counter, value);
}

template <class V>
__device__ __forceinline__ void block_append_bits(int64_t tile0, uint32_t bits,
                                                  int32_t* __restrict__ list,
                                                  int32_t* __restrict__ counter, V value) {
  __shared__ int s_wsum[kBlock / 64];
  __shared__ int s_base;
  const int c = __popc(bits);
  // block exclusive scan of c
  const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wsum[w] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int v = 0; v < kBlock / 64; ++v) {
    const int t = s_wsum[v];
    before += (v < w) ? t : 0;
    total += t;
  }
  if (threadIdx.x == 0) s_base = total ? atomicAdd(counter, total) : 0;
  __syncthreads();
  int o = s_base + before + incl - c;
  while (bits) {
    const int k = __ffs(bits) - 1;
    bits &= bits - 1;
    list[o++] = value(tile0 + (int64_t)k * kBlock + threadIdx.x);
  }
  __syncthreads();  // s_wsum / s_base reuse by the next tile
}

// ---------------------------------------------------------------- candidate windows
// The cells that may hold a neighbour: +-2 cells in space (fixed 5-wide extents so candidate
// decoding divides by constants; out-of-grid candidates are skipped) over the slabs whose actual
// time range comes within eps_t of [tlo, thi] (the +-1-slab slack window is shrunk up front with
// the per-slab time ranges).
struct Window {
  int s0, x0, y0, z0;
  int nS;
  int total;
};

__device__ __forceinline__ bool slab_in_reach(const float2* __restrict__ slab_t, int s, float tlo,
                                              float thi, float epst) {
  const float2 sr = slab_t[s];
  if (sr.x > sr.y) return false;  // empty slab
  const float gap = (tlo > sr.y) ? (tlo - sr.y) : ((thi < sr.x) ? (sr.x - thi) : 0.f);
  return gap <= epst;
}

template <int D, bool SHRINK = true>
__device__ __forceinline__ Window make_window(int cx, int cy, int cz, float tlo, float thi,
                                              const Geom& g, const float2* __restrict__ slab_t,
                                              int s_min = 0) {
  constexpr int PER = (D == 3) ? 125 : 25;
  Window w;
  const double et = (double)g.epst;
  int s0, s1;
  if (g.rt >= 0) {  // integral times: the slabs of tlo / thi (exact) +- rt
    s0 = max(slab_of(tlo, g) - g.rt, s_min);
    s1 = min(slab_of(thi, g) + g.rt, g.nt - 1);
  } else {
    s0 = (int)fmax(floor(((double)tlo - et - g.ot) * g.inv_ct) - 1.0, (double)s_min);
    s1 = (int)fmin(floor(((double)thi + et - g.ot) * g.inv_ct) + 1.0, (double)(g.nt - 1));
  }
  // shrink to the slabs in reach: one lane per slab (independent loads), ballot (callers are
  // whole waves with uniform arguments)
  const int lane = threadIdx.x & 63;
  int lo = -1, hi = -1;
  if (!SHRINK) {  // callers that classify every candidate's time range themselves
    lo = s0;
    hi = s1;
  }
  for (int c = s0; SHRINK && c <= s1; c += 64) {
    const bool ok = (c + lane <= s1) && slab_in_reach(slab_t, c + lane, tlo, thi, g.epst);
    const uint64_t m = __ballot(ok);
    if (m) {
      if (lo < 0) lo = c + __ffsll((unsigned long long)m) - 1;
      hi = c + 63 - __clzll((long long)m);
    }
  }
  if (lo < 0) {
    s0 = 0;
    s1 = -1;
  } else {
    s0 = lo;
    s1 = hi;
  }
  w.s0 = s0;
  w.nS = max(s1 - s0 + 1, 0);
  w.x0 = cx - 2;
  w.y0 = cy - 2;
  w.z0 = (D == 3) ? cz - 2 : 0;
  w.total = w.nS * PER;
  return w;
}

// make_window<D, false> of a point of slab s on integral times (g.rt >= 0), from the slab itself
// (xy points carry no time; slab_of(t) of a point is its key's slab)
template <int D>
__device__ __forceinline__ Window slab_window(int cx, int cy, int cz, int s, const Geom& g) {
  Window w;
  w.s0 = max(s - g.rt, 0);
  w.nS = max(min(s + g.rt, g.nt - 1) - w.s0 + 1, 0);
  w.x0 = cx - 2;
  w.y0 = cy - 2;
  w.z0 = (D == 3) ? cz - 2 : 0;
  w.total = w.nS * ((D == 3) ? 125 : 25);
  return w;
}

template <int D>
__device__ __forceinline__ void decode_key(int64_t key, const Geom& g, int& cx, int& cy, int& cz) {
  // keys of real cells are < 2^30 (cmax): 32-bit divisions, not the 64-bit ones' call sequence
  int cs;
  g.split((uint32_t)key, cx, cy, cz, cs);
  if (D != 3) cz = 0;
}

// q-th cell of the window; -1 when outside the grid or its slab holds nothing within reach
template <int D>
__device__ __forceinline__ int64_t window_cell(const Window& w, int q, const Geom& g,
                                               const float2* __restrict__ slab_t, float tlo,
                                               float thi) {
  constexpr int PER = (D == 3) ? 125 : 25;
  const int ss = q / PER;
  int r = q - ss * PER;
  int zz = 0;
  if (D == 3) {
    zz = r / 25;
    r -= zz * 25;
  }
  const int yy = r / 5, xx = r - yy * 5;
  const int x = w.x0 + xx, y = w.y0 + yy, z = w.z0 + zz;
  if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || (D == 3 && (z < 0 || z >= g.nz))) return -1;
  // slabs between the first and last in reach are in reach unless empty (then so are their
  // cells); the cell box's own time range is checked by classify
  const int sl = w.s0 + ss;
  return (((int64_t)sl * g.nz + z) * g.ny + y) * g.nx + x;
}

template <bool XY = false>
__device__ __forceinline__ float4 shfl_f4(const float4& v, int l) {
  if constexpr (XY) return make_float4(__shfl(v.x, l), __shfl(v.y, l), NAN, NAN);
  return make_float4(__shfl(v.x, l), __shfl(v.y, l), __shfl(v.z, l), __shfl(v.w, l));
}

// Box-box classification of two cells with the pair test's rounding (monotone bounds):
// 0 no pair can be adjacent, 1 every pair is adjacent, 2 undecided.
// SCREEN: float32 bounds first, float64 only near the threshold (Geom::e2lo / e2hi) -- faster
// in the K5 cell pass; the union kernels measured slower with it (their loops schedule worse).
template <int D, bool SCREEN = false>
__device__ __forceinline__ int classify_cells(const float4& A1, const float4& B1,
                                              const float4& A2, const float4& B2,
                                              const Geom& g) {
  // interval gap: max(b0 - a1, a0 - b1, 0) (one v_max3; equal to the branchy form, since a
  // float32 difference has the sign of the exact one)
  auto gap = [](float a0, float a1, float b0, float b1) -> float {
    return fmaxf(fmaxf(b0 - a1, a0 - b1), 0.f);
  };
  auto gapd = [](float a0, float a1, float b0, float b1) -> double {
    return (b0 > a1) ? ((double)b0 - (double)a1) : ((a0 > b1) ? ((double)a0 - (double)b1) : 0.0);
  };
  float tm = 0.f;  // (tfree: every pair of the window is within eps_t)
  if (!g.tfree) {  // kernel-uniform
    const float tg = gap(A2.z, A2.w, B2.z, B2.w);
    if (!(tg <= g.epst)) return 0;
    tm = fmaxf(fabsf(B2.w - A2.z), fabsf(A2.w - B2.z));
  }
  if (D == 2 && SCREEN) {
    const float fx = gap(A1.x, A1.y, B1.x, B1.y), fy = gap(A1.z, A1.w, B1.z, B1.w);
    const float fmn = fx * fx + fy * fy;
    const float ux = fmaxf(fabsf(B1.y - A1.x), fabsf(A1.y - B1.x));
    const float uy = fmaxf(fabsf(B1.w - A1.z), fabsf(A1.w - B1.z));
    const float fmx = ux * ux + uy * uy;
    if (fmn > g.e2hi) return 0;
    if (fmx <= g.e2lo) return (tm <= g.epst) ? 1 : 2;
    if (fmn <= g.e2lo && fmx > g.e2hi) return 2;
  }
  const double gx = gapd(A1.x, A1.y, B1.x, B1.y), gy = gapd(A1.z, A1.w, B1.z, B1.w);
  double dmin = gx * gx + gy * gy;
  const double mx = fmax(fabs((double)B1.y - (double)A1.x), fabs((double)A1.y - (double)B1.x));
  const double my = fmax(fabs((double)B1.w - (double)A1.z), fabs((double)A1.w - (double)B1.z));
  double dmax = mx * mx + my * my;
  if (D == 3) {
    const double gz = gapd(A2.x, A2.y, B2.x, B2.y);
    dmin = dmin + gz * gz;
    const double mz = fmax(fabs((double)B2.y - (double)A2.x), fabs((double)A2.y - (double)B2.x));
    dmax = dmax + mz * mz;
  }
  if (!(dmin <= g.eps2)) return 0;
  return (dmax <= g.eps2 && tm <= g.epst) ? 1 : 2;
}

// Tuning flags of the union kernels (RPT_UF_FLAGS in the A/B build): bit 0 = finds inside the
// union kernels do not path-halve (agent-scope stores drop the line from the XCD's L2; k_compress
// compresses afterwards); bit 1 = XCD-aware item ranges (blockIdx % 8 = XCD under round-robin
// placement: each XCD unions a contiguous range of cells, so its L2 keeps their parents).
// XcdRange is also the item split of the K5 / K7 queue kernels.
struct XcdRange {
  int64_t first, step, end;
};
__device__ __forceinline__ XcdRange xcd_items(int64_t n_items, bool remap) {
  const int64_t wpb = kBlock / 64, wave = threadIdx.x / 64;
  if (!remap || (gridDim.x & 7)) {
    return XcdRange{(int64_t)blockIdx.x * wpb + wave, (int64_t)gridDim.x * wpb, n_items};
  }
  const int64_t x = blockIdx.x & 7, lb = blockIdx.x >> 3, nbx = gridDim.x >> 3;
  const int64_t lo = n_items * x / 8, hi = n_items * (x + 1) / 8;
  return XcdRange{lo + lb * wpb + wave, nbx * wpb, hi};
}

// core flags v of the points [b, e) of one cell, by `lanes` lanes (j = this lane's index): bytes at
// the unaligned ends, dwords inside (cells list their points contiguously in sorted order)
__device__ __forceinline__ void write_cell_flags(uint8_t* __restrict__ core, int b, int e, int j,
                                                 int lanes, uint8_t v) {
  const int wb = (b + 3) & ~3, we = e & ~3;
  if (wb >= we) {
    for (int s = b + j; s < e; s += lanes) core[s] = v;
    return;
  }
  for (int s = b + j; s < wb; s += lanes) core[s] = v;
  const uint32_t vv = v ? 0x01010101u : 0u;
  for (int w = wb + 4 * j; w < we; w += 4 * lanes) *reinterpret_cast<uint32_t*>(core + w) = vv;
  for (int s = we + j; s < e; s += lanes) core[s] = v;
}

constexpr int kR = 4;  // candidate cells per lane per super-round of the window scans
static_assert(kR >= 2, "the union passes' candidate masks cover two 64-position rounds");
// k_union_cells: the top bit of a cell's candidate mask = "not recorded, enumerate the window"
constexpr uint32_t kPmaskFull = 0x80000000u;

constexpr int kCwMaxR = 3;
constexpr int kPU = 8;
