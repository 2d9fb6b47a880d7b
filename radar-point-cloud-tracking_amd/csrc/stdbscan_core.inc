// ST-DBSCAN stage K5, the core flags: launched by DbscanState::core_pass.  Reads
// stdbscan_shared.inc only.
// Reads occ / n_occ_dev, occ_bits, the cell records, mutual, cell_start, slab_t, skey, sorig and
// the sorted points.  Leaves behind core (one flag per sorted point) and, on the eight-lane
// (oct) paths, the per-cell (min core original index, its sorted index) pairs in cell_min_pair
// (DbscanState::cmin_ready).  Its scratch is rebuilt by the later stages: the cell flags in rep,
// the cell queue in ccmin, the point queue in nc_list, the counters at cid[n] / nc_list[n], and
// the masked path's pmask / cid per occupied cell.
// Neighbour count with early exit at min_samples; whole-cell accept/reject:
//   2-D, at most kCwMaxR slabs each side: k_core_cells_oct, then k_core_slow_masked (or
//     k_core_slow) over the queued points
//   otherwise k_core_cell_fast, k_core_cell_window, k_core_fill, k_core_slow

// ---------------------------------------------------------------- K5: core flags
// Level 1, one thread per occupied cell: a mutual cell (every pair adjacent) holding >=
// min_samples points is all core — the bulk of a radar stack.  Every other cell is queued for
// level 2 (the queue holds cell keys).  cflag (int32 per cell): 1 all core, 0 none, 2 decided
// per point (level 4).
__global__ __launch_bounds__(kBlock) void k_core_cell_fast(const int32_t* __restrict__ occ,
                                                          const int32_t* __restrict__ n_occ,
                                                          Geom g,
                                                          const int32_t* __restrict__ cell_start,
                                                          const uint8_t* __restrict__ mutual,
                                                          int32_t* __restrict__ cflag,
                                                          int32_t* __restrict__ queue,
                                                          int32_t* __restrict__ n_queue) {
  const int need = g.min_samples;
  const int64_t no = *n_occ;
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < no;
       tile += (int64_t)gridDim.x * kBlock * kItems) {
    block_append(
        tile, no,
        [&](int64_t q) -> bool {
          const int32_t c = occ[q];
          if ((int64_t)c >= g.cells || need <= 0) {  // non-finite time: no neighbours at all
            cflag[c] = (need <= 0) ? 1 : 0;
            return false;
          }
          if (mutual[c] && cell_start[c + 1] - cell_start[c] >= need) {
            cflag[c] = 1;
            return false;
          }
          return true;
        },
        queue, n_queue, [&](int64_t q) -> int32_t { return occ[q]; });
  }
}

// Level 2, one wave per queued cell A: lanes classify A's candidate cells against A's box
// (classify_cells: the pair test's rounding, monotone bounds).  Cells adjacent to every point of
// A give a count shared by all of A's points (a lower bound, self included); cells that may hold
// a neighbour give an upper bound.  Most sparse cells are decided here (flag 1 or 0) without
// touching a point; the rest get flag 2.
template <int D>
__global__ __launch_bounds__(kBlock) void k_core_cell_window(Geom g,
                                                            const int32_t* __restrict__ occ,
                                                            const CellRec<D>* __restrict__ crec,
                                                            const uint32_t* __restrict__ occ_bits,
                                                            const float2* __restrict__ slab_t,
                                                            const int32_t* __restrict__ queue,
                                                            const int32_t* __restrict__ n_queue,
                                                            int32_t* __restrict__ cflag) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  const int64_t nq = *n_queue;
  const int need = g.min_samples;
  for (int64_t q = w0; q < nq; q += nw) {
    const int32_t ca = queue[q];
    const CellRec<D> ra = crec[ca];
    const float4 A1 = rec_boxA<D>(ra), A2 = rec_boxB(ra);
    int cx, cy, cz;
    decode_key<D>(ca, g, cx, cy, cz);
    const Window w = make_window<D, true>(cx, cy, cz, A2.z, A2.w, g, slab_t);
    int lo = 0, hi = 0;
    for (int base = 0; base < w.total && lo < need; base += 64 * kR) {
      int64_t c[kR];
      uint32_t wb[kR];
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int qq = base + r * 64 + lane;
        c[r] = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, A2.z, A2.w) : -1;
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) wb[r] = (c[r] >= 0) ? occ_bits[c[r] >> 5] : 0u;
      int l = 0, h = 0;
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        if (c[r] >= 0 && ((wb[r] >> (c[r] & 31)) & 1u)) {
          const CellRec<D> cr = crec[c[r]];
          const int cls = classify_cells<D>(A1, rec_boxA<D>(cr), A2, rec_boxB(cr), g);
          l += (cls == 1) ? cr.e - cr.b : 0;
          h += (cls != 0) ? cr.e - cr.b : 0;
        }
      }
      lo += wave_sum(l);
      hi += wave_sum(h);
    }
    // an early exit leaves hi partial, but lo >= need already decides
    if (lane == 0) cflag[ca] = (lo >= need) ? 1 : ((hi < need) ? 0 : 2);
  }
}

// Row of mask position k (0..4, own row first: dy = 0, -1, +1, -2, +2) as dy + 2, branch-free
// (3-bit fields of one constant): 2, 1, 3, 0, 4.
__device__ __forceinline__ int cw_row(int k) {
  return (int)__builtin_amdgcn_ubfe(16586u, (uint32_t)(3 * k), 3u);
}

// The FUSED epilogue of k_core_cells_oct (whole wave, wave-uniform control): lanes 8k hold cell k
// of the wave (act, key, point range [b, e), flag 0 / 1 / 2).  The cells' (min original, sorted)
// pairs over ALL their points come from k_cell_box (allmin): an all-core cell keeps it, every other
// cell is reset to none here (the undecided cells' core points are folded in by k_core_slow).
// The queued points go to the block's LDS queue (an LDS atomic per wave; one global atomic per
// BLOCK when the block flushes it at its end -- a global same-address atomic per wave serialised
// ~100 k of them at 1000 frames: +0.8 ms); a wave whose points no longer fit reserves globally.
constexpr int kCwQueue = 2048;
struct CwQueue {
  int32_t item[kCwQueue];
  int32_t key[kCwQueue];  // the queued point's cell key (k_core_slow skips its skey read)
  int n;      // reserved (may pass kCwQueue)
  int fail;   // first reservation that did not fit
  int base;
};
__device__ __forceinline__ void cells_fill_epilogue(const Geom& g, bool act, int32_t ca,
                                                    int32_t qk, int b, int e, int flag,
                                                    uint8_t* __restrict__ core,
                                                    unsigned long long* __restrict__ cmin,
                                                    int32_t* __restrict__ slow,
                                                    int32_t* __restrict__ slowk,
                                                    int32_t* __restrict__ n_slow, CwQueue& lq) {
  const int lane = threadIdx.x & 63;
  if (act && (lane & 7) == 0 && flag != 1 && (int64_t)ca < g.cells) cmin[ca] = ~0ull;
  // active cells are a prefix of the eight (occupied-list positions below the range end)
  const int na = __popcll(__ballot(act && (lane & 7) == 0));
  if (na == 0) return;
  int gb[8], gf[8], gc[8];
  int E = 0, nu = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gb[k] = __builtin_amdgcn_readlane(b, 8 * k);
    gc[k] = __builtin_amdgcn_readlane(qk, 8 * k);  // the queue's per-point cell word
    const int ek = __builtin_amdgcn_readlane(e, 8 * k);
    gf[k] = __builtin_amdgcn_readlane(flag, 8 * k);
    if (k < na) {
      E = ek;
      nu += (gf[k] == 2) ? ek - gb[k] : 0;
    }
  }
  const int B = gb[0];
  int ub = 0;
  int32_t* qdst = lq.item;
  int32_t* kdst = lq.key;
  if (nu > 0) {  // the undecided cells' points: one queue reservation per wave
    if (lane == 0) {
      ub = atomicAdd(&lq.n, nu);
      if (ub + nu > kCwQueue) {
        atomicMin(&lq.fail, ub);
        ub = -1 - atomicAdd(n_slow, nu);
      }
    }
    ub = __shfl(ub, 0);
    if (ub < 0) {
      qdst = slow;
      kdst = slowk;
      ub = -1 - ub;
    }
  }
  const uint64_t below = (1ull << lane) - 1ull;
  for (int s0 = B; s0 < E; s0 += 64) {
    const int s = s0 + lane;
    const bool in = s < E;
    int fl = gf[0], c = gc[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const bool sel = k < na && s >= gb[k];
      fl = sel ? gf[k] : fl;
      c = sel ? gc[k] : c;
    }
    const bool u = in && fl == 2;
    const uint64_t um = nu > 0 ? __ballot(u) : 0ull;
    if (u) {
      const int o = ub + __popcll(um & below);
      qdst[o] = s;
      kdst[o] = c;
    }
    ub += __popcll(um);
    if (in) core[s] = (fl == 1) ? 1 : 0;
  }
}

// 2-D grids whose slab window is at most 7 slabs (R <= 3): K5 levels 1-3 in one kernel, EIGHT
// lanes per occupied cell.  A mutual cell with >= min_samples points is all core (the bulk);
// otherwise lane j < 2R+1 owns slab cs - R + j of the cell's window.  The window comes from the
// cell's slab alone (R = ceil(eps_t / slab) + 1 slabs each side, pruned with the slabs' actual
// time ranges), so a lane loads its slab's range and the occupancy words of its 5 rows together
// with the cell's record, then the records of its (few) occupied candidates; eight cells per wave
// keep many short dependency chains in flight.  cflag as k_core_cell_fast / _window (level 3
// turns it into point flags).
//
// FUSED (the default pipeline): the level-3 fill folded in.  A wave's eight cells are consecutive
// occupied cells, so their points are ONE contiguous range of the sorted order (the cells between
// consecutive occupied keys are empty); after the decisions the whole wave walks that range 64
// points at a time: the point flags (byte stores, 64 consecutive bytes per instruction) and the
// undecided cells' points appended to the level-4 queue (one atomic per wave).  The all-core
// cells' (min original, sorted) pairs are k_cell_box's (allmin).  No per-point loads at all.
// Sum over each aligned group of eight lanes, every lane of the group getting it (row_reduce:
// DPP, no LDS round trips).  Every lane of a group must be active (the cell kernels' branches
// are group-uniform).
__device__ __forceinline__ int sum8(int v) { return row_reduce<8>(v, OpAdd{}); }

constexpr int kCwBatch = 4;  // candidate records per lane in flight together (k_core_cells_oct)
// MASK (with FUSED, windows of W = 2R + 1 <= 5 slabs): every undecided cell hands its decisions
// to k_core_slow_masked -- its whole-accept count lo (clo[q], q = its occupied-list position) and
// the 128-bit mask of its candidates that box classification left partial (pmask[q]; window
// position 5 P + dx, P = the (slab, row) pair j + 8 i of lane j's slot i) -- and queues its points
// with q instead of the cell key.
template <bool FUSED = false, bool MASK = false>
// 5 waves/SIMD (<= 96 VGPRs; the fused epilogue and its LDS queue would take 99: 4 waves)
__global__ __launch_bounds__(kBlock, 5) void k_core_cells_oct(Geom g, int R,
                                                          const int32_t* __restrict__ occ,
                                                          const int32_t* __restrict__ n_occ,
                                                          const CellRec<2>* __restrict__ crec,
                                                          const uint8_t* __restrict__ mutual,
                                                          const uint32_t* __restrict__ occ_bits,
                                                          const float2* __restrict__ slab_t,
                                                          int32_t* __restrict__ cflag,
                                                          int32_t* __restrict__ zero_counter,
                                                          uint8_t* __restrict__ core,
                                                          unsigned long long* __restrict__ cmin =
                                                              nullptr,
                                                          int32_t* __restrict__ slow = nullptr,
                                                          int32_t* __restrict__ slowk = nullptr,
                                                          int32_t* __restrict__ n_slow = nullptr,
                                                          uint4* __restrict__ pmask = nullptr,
                                                          int32_t* __restrict__ clo = nullptr) {
  static_assert(!MASK || FUSED, "the masks feed the fused pipeline's slow pass");
  // legacy pipeline: the level-4 queue counter, zeroed here instead of by a memset launch
  // (k_core_fill, the next kernel on the stream, is its first user)
  if (!FUSED && zero_counter && blockIdx.x == 0 && threadIdx.x == 0) *zero_counter = 0;
  __shared__ CwQueue lq;
  // per lane its five (slab, row) slots' keys of column dx = 0, written once per cell and read
  // per candidate (recomputing them took ~20 VALU per candidate, three 32-bit multiplies among
  // them; five more registers spilled)
  __shared__ int32_t s_k0[5][kBlock];
  if (FUSED) {
    if (threadIdx.x == 0) {
      lq.n = 0;
      lq.fail = kCwQueue;
    }
    __syncthreads();
  }
  const int64_t no = *n_occ;
  const int need = g.min_samples;
  const int j = threadIdx.x & 7;
  // XCD-aware cell ranges (grid a multiple of 8): blocks sharing an XCD take one contiguous
  // eighth of the (slab-major) occupied cells, so the neighbouring slabs' records they read stay
  // in that XCD's L2 instead of being fetched by all eight
  const int64_t cpb = blockDim.x / 8;
  const int64_t xg = blockIdx.x & 7, nbx = gridDim.x >> 3;
  const int64_t qlo = no * xg / 8, qhi = no * (xg + 1) / 8;
  for (int64_t q0 = qlo + (int64_t)(blockIdx.x >> 3) * cpb; q0 < qhi; q0 += nbx * cpb) {
    const int64_t q = q0 + threadIdx.x / 8;
    const bool act = q < qhi;
    const int32_t ca = act ? occ[q] : 0;
    int flag = 0, b = 0, e = 0;
    if (act && (int64_t)ca >= g.cells) {  // non-finite time: no neighbours at all
      flag = (need <= 0) ? 1 : 0;
      const CellRec<2> ri = crec[ca];
      b = ri.b;
      e = ri.e;
    } else if (act) {
      int cx, cy, cz, cs;
      g.split((uint32_t)ca, cx, cy, cz, cs);
      // window of W = 2R + 1 slabs; lane j < W tests the time reach of slab cs - R + j
      const int W = 2 * R + 1;
      const int sl = cs + j - R;
      const bool sv = j < W && sl >= 0 && sl < g.nt;
      const CellRec<2> ra = crec[ca];
      const uint8_t mu = mutual[ca];
      b = ra.b;
      e = ra.e;
      const float2 own = slab_t[cs];
      float2 sr = make_float2(1.f, 0.f);
      // The window's 5 W (slab, row) pairs are spread over ALL eight lanes of the cell: pair
      // p = k W + si (row rank k: dy = 0, -1, +1, -2, +2, own row first; slab index si) is slot
      // p / 8 of lane p % 8.  (A lane per slab left 8 - W lanes idle through the candidate loop
      // -- 3 of 8 at the usual W = 5 -- and the busiest slab set the loop's trip count.)
      uint32_t m5[5];  // slot i: occupied columns dx = 0..4 of its row (x = cx - 2 + dx)
      int psi[5];      // slot i: slab index
      const uint32_t mg = (65535u + (uint32_t)W) / (uint32_t)W;  // p / W = (p * mg) >> 16
      {
        // branch-free: an invalid slot reads a valid word and masks it off, so all eleven loads
        // of every lane are in flight together (a conditional load is a branch ending in a full
        // vmcnt wait)
        const int slc = sv ? sl : cs;
        const float2 srv = slab_t[slc];
        sr = sv ? srv : sr;
        const int lo_x = cx - 2 < 0 ? 2 - cx : 0;
        const int hi_x = cx + 2 - (g.nx - 1);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int p = j + 8 * i;
          const int k = min((int)(((uint32_t)p * mg) >> 16), 4);
          const int si = p - k * W;
          const int s2 = cs + si - R;
          const int y = cy + cw_row(k) - 2;
          const bool v = p < 5 * W && s2 >= 0 && s2 < g.nt && y >= 0 && y < g.ny;
          // (int32 keys: cells < 2^30)
          const int k0 = ((v ? s2 : cs) * g.ny + (v ? y : cy)) * g.nx + (cx - 2);
          s_k0[i][threadIdx.x] = k0;  // column dx = 0 of slot i (the lane's own LDS words)
          const int kk = k0 < 0 ? 0 : k0;
          const int w = kk >> 5;
          const uint32_t lo_w = occ_bits[w], hi_w = occ_bits[w + 1];
          uint32_t m = (k0 < 0) ? ((lo_w << (-k0)) & 31u)
                                : (__builtin_amdgcn_alignbit(hi_w, lo_w, (uint32_t)(kk & 31)) & 31u);
          m &= ~((1u << lo_x) - 1u);
          if (hi_x > 0) m &= (31u >> hi_x);
          m5[i] = v ? m : 0u;
          psi[i] = v ? si : 0;
        }
      }
      const float gap =
          (own.x > sr.y) ? (own.x - sr.y) : ((sr.x > own.y) ? (sr.x - own.y) : 0.f);
      const bool reach = sv && sr.x <= sr.y && gap <= g.epst;  // slab j is in reach
      // the cell's reach bits (slab index -> bit), from its eight lanes (group-uniform branch)
      const uint32_t rbits =
          (uint32_t)(__ballot(reach) >> (threadIdx.x & 56)) & 0xffu;
      // the lane's occupied candidates as one 25-bit mask, slot-major (bits 5i .. 5i + 4 = slot
      // i's columns): rows nearest first
      uint32_t m25 = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) m25 |= (((rbits >> psi[i]) & 1u) ? m5[i] : 0u) << (5 * i);
      if (need <= 0 || (mu && e - b >= need)) {
        flag = 1;
      } else {
        int lo = 0, hi = 0;
        const float4 A1 = rec_boxA<2>(ra), A2 = rec_boxB(ra);
        // taken kCwBatch at a time with all their record loads in flight together: a sparse
        // cell's few candidates cost ONE round trip instead of one per row; the eight lanes stop
        // as soon as the adjacent-to-every-point count reaches min_samples (dense cells: after
        // the own row's batch)
        bool decided = false;
        uint32_t pm25 = 0;  // (MASK) the lane's candidates left partial, bits as m25's
        while (true) {
          int rem = m25 ? 1 : 0;
          rem = sum8(rem);
          if (rem == 0) break;  // (uniform over the cell's eight lanes)
          CellRec<2> cr[kCwBatch];
          bool has[kCwBatch];
          const uint32_t mb = m25;  // (MASK) the batch takes the lowest set bits of mb
#pragma unroll
          for (int i = 0; i < kCwBatch; ++i) {
            // branch-free record loads (a lane without a candidate re-reads its own cell's)
            has[i] = m25 != 0;
            const int p = __builtin_ctz(m25 | (1u << 31));
            m25 &= m25 - 1;
            const int sl5 = (p * 13) >> 6;  // slot p / 5 (p < 32)
            const int key = s_k0[sl5][threadIdx.x] + (p - 5 * sl5);
            cr[i] = crec[has[i] ? key : ca];
          }
          uint32_t pf = 0;  // (MASK) batch entries left partial
#pragma unroll
          for (int i = 0; i < kCwBatch; ++i) {
            if (!has[i]) continue;
            const int cls =
                classify_cells<2, true>(A1, rec_boxA<2>(cr[i]), A2, rec_boxB(cr[i]), g);
            lo += (cls == 1) ? cr[i].e - cr[i].b : 0;
            hi += (cls != 0) ? cr[i].e - cr[i].b : 0;
            if (MASK) pf |= (cls == 2) ? (1u << i) : 0u;
          }
          if (MASK) {
            uint32_t tk = mb & ~m25;  // entry i = the i-th lowest bit taken
#pragma unroll
            for (int i = 0; i < kCwBatch; ++i) {
              pm25 |= ((pf >> i) & 1u) ? (tk & (0u - tk)) : 0u;
              tk &= tk - 1;
            }
          }
          int ls = lo;
          ls = sum8(ls);
          if (ls >= need) {
            decided = true;
            break;
          }
        }
        if (decided) {
          flag = 1;
        } else {
          lo = sum8(lo);
          hi = sum8(hi);
          flag = (lo >= need) ? 1 : ((hi < need) ? 0 : 2);
          if (MASK && flag == 2) {  // (group-uniform) hand the decisions to the slow pass
            // slot i of lane j = pair P = j + 8 i; its five columns go to window positions
            // 5 P .. 5 P + 4 (P < 5 W <= 25: slot 4 and most of slot 3 are never valid)
            uint64_t mlo = 0, mhi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const uint64_t ch = (pm25 >> (5 * i)) & 31u;
              const int pos = 5 * (j + 8 * i);
              if (pos < 64) {
                mlo |= ch << pos;
                if (pos > 59) mhi |= ch >> (64 - pos);
              } else if (pos < 128) {
                mhi |= ch << (pos - 64);
              }
            }
            mlo = row_reduce<8>(mlo, OpOr{});
            mhi = row_reduce<8>(mhi, OpOr{});
            if (j == 0) {
              pmask[q] = make_uint4((uint32_t)mlo, (uint32_t)(mlo >> 32), (uint32_t)mhi,
                                    (uint32_t)(mhi >> 32));
              clo[q] = lo;
            }
          }
        }
      }
    }
    if constexpr (!FUSED) {
      if (act && j == 0) cflag[ca] = flag;
      // decided cells write their points' flags here (the undecided ones are k_core_slow_cells')
      if (core && act && flag != 2) write_cell_flags(core, b, e, j, 8, (uint8_t)flag);
    } else {
      // (MASK: the queue carries the cell's occupied-list position instead of its key)
      cells_fill_epilogue(g, act, ca, MASK ? (int32_t)q : ca, b, e, flag, core, cmin, slow, slowk,
                          n_slow, lq);
    }
  }
  if constexpr (FUSED) {  // flush the block's queue (the cell loop is block-uniform)
    __syncthreads();
    const int m = min(lq.n, lq.fail);
    if (threadIdx.x == 0) lq.base = m > 0 ? atomicAdd(n_slow, m) : 0;
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
      slow[lq.base + i] = lq.item[i];
      slowk[lq.base + i] = lq.key[i];
    }
  }
}

// Level 3, one thread per point: the cell's decision; points of undecided cells are queued for
// level 4 (block-aggregated append; QUEUE = false: the undecided cells are left to
// k_core_slow_cells).
// cmin (nullable, ~0 for the occupied cells): the union's per-cell (min original, sorted) pair
// of the core points (k_cell_min_pair folded in): all-core cells here, by a segmented wave
// minimum over the sorted points; the undecided cells' core points in k_core_slow.
template <bool QUEUE>
__global__ __launch_bounds__(kBlock) void k_core_fill(const int32_t* __restrict__ skey, int64_t n,
                                                     const int32_t* __restrict__ cflag,
                                                     uint8_t* __restrict__ core,
                                                     int32_t* __restrict__ slow,
                                                     int32_t* __restrict__ n_slow,
                                                     const int32_t* __restrict__ sorig = nullptr,
                                                     unsigned long long* __restrict__ cmin =
                                                         nullptr,
                                                     int64_t cells = 0) {
  const int lane = threadIdx.x & 63;
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < n;
       tile += (int64_t)gridDim.x * kBlock * kItems) {
    // all keys, then all cell flags, in flight together (two rounds of memory latency per tile,
    // not two per item)
    // branch-free (clamped indices, results masked): each level's loads in flight together
    int32_t key[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      const int32_t kv = skey[min(s, n - 1)];
      key[k] = (s < n) ? kv : -1;
    }
    int f[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int32_t fv = cflag[key[k] >= 0 ? key[k] : 0];
      f[k] = (key[k] >= 0) ? fv : 0;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      if (s < n) core[s] = (f[k] == 1) ? 1 : 0;
      bits |= (f[k] == 2) ? (1u << k) : 0u;
    }
    if (cmin) {  // kernel-uniform
      uint32_t so[kItems];
#pragma unroll
      for (int k = 0; k < kItems; ++k) {
        const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
        so[k] = (f[k] == 1 && s < n) ? (uint32_t)sorig[s] : 0u;
      }
#pragma unroll
      for (int k = 0; k < kItems; ++k) {
        const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
        const int kk = key[k];
        // sorted keys: a run of equal keys is one cell; dist = lanes since this lane's run head
        const int prevk = __shfl_up(kk, 1, 64), next = __shfl_down(kk, 1, 64);
        const uint64_t hm = __ballot(lane == 0 || prevk != kk);
        const uint64_t upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const int dist = lane - (63 - __builtin_clzll(hm & upto));
        const bool in = f[k] == 1 && kk >= 0 && (int64_t)kk < cells;
        const bool tail = (lane == 63 || next != kk) && kk >= 0;
        if (n < (int64_t(1) << 26)) {  // kernel-uniform: (original << 6 | lane) fits 32 bits
          uint32_t v = in ? ((so[k] << 6) | (uint32_t)lane) : ~0u;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)v, off, 64);
            if (off <= dist) v = min(v, o);
          }
          if (tail && v != ~0u)
            atomicMin(cmin + kk, ((unsigned long long)(v >> 6) << 32) |
                                     (uint32_t)(s - lane + (int)(v & 63u)));
        } else {
          uint64_t v = in ? (((uint64_t)so[k] << 32) | (uint32_t)s) : ~0ull;
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const uint32_t olo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
            const uint32_t ohi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64);
            if (off <= dist) v = min(v, ((uint64_t)ohi << 32) | olo);
          }
          if (tail && v != ~0ull) atomicMin(cmin + kk, (unsigned long long)v);
        }
      }
    }
    if (QUEUE) block_append_bits(tile, bits, slow, n_slow);
  }
}

// Level 4, one wave per queued point: lanes classify up to 64 candidate cells at a time against
// the cells' boxes (whole-cell accept adds the cell's count), then every undecided cell's points
// are tested 64 at a time; the wave stops as soon as min_samples neighbours are seen.
template <int D, int KR = kR>
// KR: candidate positions per lane per super-round (2 when the exact integral-time window of
// (2 rt + 1) x 25 positions fits 128: the other two rounds only masked positions off)
// 8 waves/SIMD (64 VGPRs, one spill; 72 gave 7): -3 % on the latency-bound queue pass
__global__ __launch_bounds__(kBlock, 8) void k_core_slow(const float4* __restrict__ pts,
                                                     const int32_t* __restrict__ skey, Geom g,
                                                     const CellRec<D>* __restrict__ crec,
                                                     const uint32_t* __restrict__ occ_bits,
                                                     const float2* __restrict__ slab_t,
                                                     const int32_t* __restrict__ slow,
                                                     const int32_t* __restrict__ n_slow,
                                                     uint8_t* __restrict__ core,
                                                     const int32_t* __restrict__ sorig = nullptr,
                                                     unsigned long long* __restrict__ cmin =
                                                         nullptr,
                                                     const int32_t* __restrict__ slowk = nullptr) {
  const int lane = threadIdx.x & 63;
  const int need = g.min_samples;
  // XCD-aware ranges of the (cell-ordered) queue: neighbouring points' windows share an L2
  const XcdRange xr = xcd_items(*n_slow, true);
  for (int64_t q = xr.first; q < xr.end; q += xr.step) {
    const int s = slow[q];
    // slowk (the fused cell pass): the key comes with the queue entry, and with integral times
    // the window is the key's slab +- rt, so the occupancy loads do not wait for the point
    const int32_t key = slowk ? slowk[q] : skey[s];
    const float4 p = pts[s];
    int cx, cy, cz;
    decode_key<D>(key, g, cx, cy, cz);
    Window w;
    if (slowk && g.rt >= 0) {  // slab_of(p.w) is the key's slab (same cell_of)
      const int cs = g.slab_of_key(key);
      w.s0 = max(cs - g.rt, 0);
      w.nS = max(min(cs + g.rt, g.nt - 1) - w.s0 + 1, 0);
      w.x0 = cx - 2;
      w.y0 = cy - 2;
      w.z0 = (D == 3) ? cz - 2 : 0;
      w.total = w.nS * ((D == 3) ? 125 : 25);
    } else {
      w = make_window<D, false>(cx, cy, cz, p.w, p.w, g, slab_t);
    }
    int cnt = 0;
    // super-rounds of KR candidates per lane: every lane's bitmap words, then records, are
    // loaded together (one dependent level each for up to 64*KR candidates)
    for (int base = 0; base < w.total && cnt < need; base += 64 * KR) {
      int64_t c[KR];
      uint32_t wb[KR];
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const int qq = base + r * 64 + lane;
        c[r] = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
      }
#pragma unroll
      for (int r = 0; r < KR; ++r) wb[r] = (c[r] >= 0) ? occ_bits[c[r] >> 5] : 0u;
      int b[KR], e[KR], cls[KR];
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        b[r] = e[r] = cls[r] = 0;
        if (c[r] >= 0 && ((wb[r] >> (c[r] & 31)) & 1u)) {
          const CellRec<D> cr = crec[c[r]];
          b[r] = cr.b;
          e[r] = cr.e;
          cls[r] = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
        }
      }
      // whole-cell accepts (lower bound) and every cell that may hold a neighbour (upper bound,
      // with the super-rounds still to come): a point whose upper bound stays below min_samples
      // is decided without a pair test
      int add = 0, may = 0;
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        add += (cls[r] == 1) ? e[r] - b[r] : 0;
        may += (cls[r] == 2) ? e[r] - b[r] : 0;
      }
      cnt += wave_sum(add);
      const bool last = base + 64 * KR >= w.total;
      if (last && cnt + wave_sum(may) < need) break;
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        uint64_t pm = __ballot(cls[r] == 2);
        while (pm && cnt < need) {
          const int l = __ffsll((unsigned long long)pm) - 1;
          pm &= pm - 1;
          const int bb = __shfl(b[r], l), ee = __shfl(e[r], l);
          for (int j0 = bb; j0 < ee && cnt < need; j0 += 64) {
            const int j = j0 + lane;
            const bool a = (j < ee) && adjacent<D>(p, pts[j], g);
            cnt += __popcll(__ballot(a));
          }
        }
      }
    }
    if (lane == 0) {
      core[s] = (cnt >= need) ? 1 : 0;
      if (cmin && cnt >= need && (int64_t)key < g.cells)
        atomicMin(cmin + key, ((unsigned long long)(uint32_t)sorig[s] << 32) | (uint32_t)s);
    }
  }
}

// Level 4 fed by the fused cell pass's decisions (k_core_cells_oct<true, true>; 2-D, W = 2R + 1
// <= 5): one wave per queued point, whose cell's candidates are already split into whole accepts
// (their count lo, exact for every point of the cell), rejects (no neighbour of any point of the
// cell) and the partial ones (pmask).  So the point starts at cnt = lo and classifies ONLY the
// partial candidates (lane l takes window positions l and l + 64 of the mask): no occupancy
// words, no record loads or box tests of the decided candidates -- then the pair tests of the
// candidates still partial for the point itself, early exit at min_samples, as k_core_slow.
__device__ __forceinline__ int mask_pos_key(int pos, const Geom& g, int R, int W, uint32_t mg,
                                            int cx, int cy, int cs) {
  const int P = pos / 5, dx = pos - 5 * P;
  const int k = min((int)(((uint32_t)P * mg) >> 16), 4);  // P / W
  const int si = P - k * W;
  const int s2 = cs + si - R;
  const int y = cy + cw_row(k) - 2;
  return (s2 * g.ny + y) * g.nx + (cx - 2 + dx);
}
template <bool XY>
__global__ __launch_bounds__(kBlock, 8) void k_core_slow_masked(
    const Pt<XY>* __restrict__ pts, Geom g, int R, const CellRec<2>* __restrict__ crec,
    const int32_t* __restrict__ occ, const int32_t* __restrict__ slow,
    const int32_t* __restrict__ slowq, const int32_t* __restrict__ n_slow,
    const uint4* __restrict__ pmask, const int32_t* __restrict__ clo, uint8_t* __restrict__ core,
    const int32_t* __restrict__ sorig, unsigned long long* __restrict__ cmin) {
  const int lane = threadIdx.x & 63;
  const int need = g.min_samples;
  const int W = 2 * R + 1;
  const uint32_t mg = (65535u + (uint32_t)W) / (uint32_t)W;
  const XcdRange xr = xcd_items(*n_slow, true);
  for (int64_t q = xr.first; q < xr.end; q += xr.step) {
    const int s = slow[q];
    const int32_t cq = slowq[q];
    // all independent of each other: one round of memory latency
    const float4 p = load_pt<XY>(pts, s);
    const int32_t key = occ[cq];
    const uint4 m = pmask[cq];
    int cnt = clo[cq];
    int cx, cy, cz, cs;
    g.split((uint32_t)key, cx, cy, cz, cs);
    const uint32_t w0 = lane < 32 ? m.x : m.y;  // positions lane, lane + 64
    const uint32_t w1 = lane < 32 ? m.z : m.w;
    const bool h0 = (w0 >> (lane & 31)) & 1u, h1 = (w1 >> (lane & 31)) & 1u;
    const int k0 = h0 ? mask_pos_key(lane, g, R, W, mg, cx, cy, cs) : key;
    const int k1 = h1 ? mask_pos_key(lane + 64, g, R, W, mg, cx, cy, cs) : key;
    const CellRec<2> c0 = crec[k0], c1 = crec[k1];  // (branch-free: the own record otherwise)
    const int cl0 = h0 ? classify<2, XY>(p, rec_boxA<2>(c0), rec_boxB(c0), g) : 0;
    const int cl1 = h1 ? classify<2, XY>(p, rec_boxA<2>(c1), rec_boxB(c1), g) : 0;
    int add = (cl0 == 1 ? c0.e - c0.b : 0) + (cl1 == 1 ? c1.e - c1.b : 0);
    int may = (cl0 == 2 ? c0.e - c0.b : 0) + (cl1 == 2 ? c1.e - c1.b : 0);
    cnt += wave_sum(add);
    if (cnt < need && cnt + wave_sum(may) >= need) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int cl = r ? cl1 : cl0;
        const int bq = r ? c1.b : c0.b, eq = r ? c1.e : c0.e;
        uint64_t pm = __ballot(cl == 2);
        while (pm && cnt < need) {
          const int l = __ffsll((unsigned long long)pm) - 1;
          pm &= pm - 1;
          const int bb = __shfl(bq, l), ee = __shfl(eq, l);
          for (int j0 = bb; j0 < ee && cnt < need; j0 += 64) {
            const int jj = j0 + lane;
            const bool a = (jj < ee) && adjacent<2, XY>(p, load_pt<XY>(pts, jj), g);
            cnt += __popcll(__ballot(a));
          }
        }
      }
    }
    if (lane == 0) {
      core[s] = (cnt >= need) ? 1 : 0;
      if (cmin && cnt >= need)
        atomicMin(cmin + key, ((unsigned long long)(uint32_t)sorig[s] << 32) | (uint32_t)s);
    }
  }
}
