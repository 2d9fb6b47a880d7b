// ST-DBSCAN stage "count", the exact neighbour counts and the core flags made from them: launched
// by DbscanState::count_pass and DbscanState::core_from_counts.  Reads stdbscan_shared.inc only.
// Reads occ / n_occ_dev, occ_bits, the cell records, slab_t, sorig and the sorted float4 points
// (never the xy layout: count_pass calls need_float4).  Leaves behind counts_sorted (one int32
// per sorted point: |{ j : adjacent(p_s, p_j) }|, s itself included, 0 for the points of the
// isolated cell) and, after core_from_counts, core (counts_sorted[s] >= m) with the number of core
// points in a pre-zeroed pool word (DbscanState::n_core_dev).  DbscanState::counts is a Budget
// line of its own (n int32) in build_t: it has to outlive every union_pass / labels_local of a
// min_samples sweep, and those rebuild all the other per-point scratch.  The only other scratch is
// the kernel's LDS list.
// No early exit and no min_samples anywhere: one kernel family, k_count_cells<2> / <3>, for
// integral and generic time windows, coarsened cells and every slab reach.
//   one wave per occupied cell A: the lanes classify the cells of A's window against A's box
//   (classify_cells, the pair test's rounding): class 1 adds the cell's point count to a base
//   shared by all of A's points (a mutual A is class 1 against itself), class 0 adds nothing,
//   class 2 goes to the wave's list in LDS; then count_listed tests A's points against the listed
//   cells' points pair by pair, in one of two lane mappings chosen by A's size.

constexpr int kCntList = 128;   // listed cells per wave between two pair phases
constexpr int kCntSmallA = 16;  // up to this many own points the lanes take CANDIDATE points
constexpr int kCntSmallB = 4;   // ... and candidate cells up to this size take one lane each
constexpr int kCntBox = 8;      // own-point lanes classify a listed cell of at least this size

// v of lane l (wave-uniform l) in every lane, by v_readlane: no LDS round trip
__device__ __forceinline__ float4 lane_f4(const float4& v, int l) {
  return make_float4(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), l)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), l)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.z), l)),
                     __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.w), l)));
}

// Lanes 0 .. nA-1 hold A's points (pa); q is this lane's candidate point (in: it is one).  Adds to
// lane i's cnt the number of lanes whose candidate is adjacent to A's point i.  Whole wave.
template <int D>
__device__ __forceinline__ void count_against_own(const float4& pa, int nA, const float4& q,
                                                  bool in, const Geom& g, int lane, int& cnt) {
  for (int i = 0; i < nA; ++i) {
    const float4 pi = lane_f4(pa, i);
    const int h = __popcll(__ballot(in && adjacent<D>(pi, q, g)));
    cnt += (lane == i) ? h : 0;
  }
}

// The pair phase of one wave: the points [b, e) of cell A against the points of the nl listed
// cells.  counts[s] = the pairs found + add (+ counts[s] when an earlier phase of this cell wrote
// its share already: prior).  All arguments but the pointers' contents are wave-uniform.
template <int D>
__device__ __forceinline__ void count_listed(const float4* __restrict__ pts, const Geom& g,
                                             const CellRec<D>* __restrict__ crec,
                                             const int32_t* list, int nl, int b, int e, int add,
                                             bool prior, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int nA = e - b;
  if (nA <= kCntSmallA) {
    // few own points (clutter, blob fringes): lane i < nA keeps A's point i and its count; the
    // candidates spread over the lanes and every own point is broadcast to them in turn
    const float4 pa = pts[b + min(lane, nA - 1)];
    int cnt = 0;
    for (int k0 = 0; k0 < nl; k0 += 64) {
      const int k = k0 + lane;
      int cb = b, cn = 0;
      if (k < nl) {
        const CellRec<D> cr = crec[list[k]];
        cb = cr.b;
        cn = cr.e - cr.b;
      }
      // small listed cells, one lane each: round r tests their r-th points together
      const bool small = cn <= kCntSmallB;
      for (int r = 0; r < kCntSmallB; ++r) {
        const bool in = small && r < cn;
        if (!__ballot(in)) break;
        const float4 q = pts[in ? cb + r : b];
        count_against_own<D>(pa, nA, q, in, g, lane, cnt);
      }
      // the others one at a time, the lanes over their points
      uint64_t big = __ballot(!small);
      while (big) {
        const int l = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        const int bb = __builtin_amdgcn_readlane(cb, l), nn = __builtin_amdgcn_readlane(cn, l);
        for (int j0 = 0; j0 < nn; j0 += 64) {
          const bool in = j0 + lane < nn;
          const float4 q = pts[in ? bb + j0 + lane : bb];
          count_against_own<D>(pa, nA, q, in, g, lane, cnt);
        }
      }
    }
    if (lane < nA) {
      const int s = b + lane;
      counts[s] = cnt + add + (prior ? counts[s] : 0);
    }
    return;
  }
  // many own points (blobs): a lane per own point, 64 at a time; every lane walks the listed
  // cells' points (uniform addresses), after a box test of its own against the larger cells
  for (int s0 = b; s0 < e; s0 += 64) {
    const int s = s0 + lane;
    const bool own = s < e;
    const float4 p = pts[own ? s : b];
    int cnt = 0;
    for (int k = 0; k < nl; ++k) {
      const CellRec<D> cr = crec[list[k]];
      const int cb = __builtin_amdgcn_readfirstlane(cr.b);
      const int ce = __builtin_amdgcn_readfirstlane(cr.e);
      int cls = 2;
      if (ce - cb >= kCntBox) cls = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
      cnt += (cls == 1) ? ce - cb : 0;
      const bool test = own && cls == 2;
      if (!__ballot(test)) continue;
      constexpr int kU = 4;  // candidate loads in flight
      for (int j0 = cb; j0 < ce; j0 += kU) {
        float4 q[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) q[u] = pts[min(j0 + u, ce - 1)];
#pragma unroll
        for (int u = 0; u < kU; ++u)
          cnt += (test && j0 + u < ce && adjacent<D>(p, q[u], g)) ? 1 : 0;
      }
    }
    if (own) counts[s] = cnt + add + (prior ? counts[s] : 0);
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_count_cells(const float4* __restrict__ pts, Geom g,
                                                       const int32_t* __restrict__ occ,
                                                       const int32_t* __restrict__ n_occ,
                                                       const CellRec<D>* __restrict__ crec,
                                                       const uint32_t* __restrict__ occ_bits,
                                                       const float2* __restrict__ slab_t,
                                                       int32_t* __restrict__ counts) {
  __shared__ int32_t s_list[kBlock / 64][kCntList];
  const int lane = threadIdx.x & 63;
  int32_t* list = s_list[threadIdx.x / 64];
  const uint64_t below = (1ull << lane) - 1ull;
  // XCD-aware ranges of the ascending occupied list: neighbouring cells' windows share an L2
  const XcdRange xr = xcd_items(*n_occ, true);
  for (int64_t q = xr.first; q < xr.end; q += xr.step) {
    const int32_t ca = occ[q];
    const CellRec<D> ra = crec[ca];
    const int b = __builtin_amdgcn_readfirstlane(ra.b), e = __builtin_amdgcn_readfirstlane(ra.e);
    if ((int64_t)ca >= g.cells) {  // non-finite times: nobody's neighbour, not even their own
      for (int s = b + lane; s < e; s += 64) counts[s] = 0;
      continue;
    }
    const float4 A1 = rec_boxA<D>(ra), A2 = rec_boxB(ra);
    int cx, cy, cz;
    decode_key<D>(ca, g, cx, cy, cz);
    const Window w = make_window<D, true>(cx, cy, cz, A2.z, A2.w, g, slab_t);
    int base = 0, nl = 0;
    bool prior = false;
    for (int q0 = 0; q0 < w.total; q0 += 64) {
      if (nl + 64 > kCntList) {  // the list may not hold this round: count what it holds
        count_listed<D>(pts, g, crec, list, nl, b, e, 0, prior, counts);
        prior = true;
        nl = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      const int qq = q0 + lane;
      const int64_t c = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, A2.z, A2.w) : -1;
      int whole = 0;
      bool part = false;
      if (c >= 0 && occupied(occ_bits, c)) {
        const CellRec<D> cr = crec[c];
        const int cls = classify_cells<D, true>(A1, rec_boxA<D>(cr), A2, rec_boxB(cr), g);
        whole = (cls == 1) ? cr.e - cr.b : 0;
        part = cls == 2;
      }
      base += wave_sum(whole);
      const uint64_t pm = __ballot(part);
      if (part) list[nl + __popcll(pm & below)] = (int32_t)c;
      nl += __popcll(pm);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    count_listed<D>(pts, g, crec, list, nl, b, e, base, prior, counts);
    // (the next cell's list writes come after this cell's reads in program order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// core[s] = counts[s] >= m, and the number of core points at *n_core (zeroed by the caller): one
// atomic per wave
__global__ __launch_bounds__(kBlock) void k_core_from_counts(const int32_t* __restrict__ counts,
                                                            int64_t n, int32_t m,
                                                            uint8_t* __restrict__ core,
                                                            int32_t* __restrict__ n_core) {
  int mine = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const bool c = counts[s] >= m;
    core[s] = c ? 1 : 0;
    mine += c ? 1 : 0;
  }
  const int tot = wave_sum(mine);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(n_core, tot);
}

// the sorted counts in original order
__global__ __launch_bounds__(kBlock) void k_counts_to_orig(const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ sorig,
                                                          int64_t n, int32_t* __restrict__ out) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    out[sorig[s]] = counts[s];
}
