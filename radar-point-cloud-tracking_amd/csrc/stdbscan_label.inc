// ST-DBSCAN stages K7/K8, component ids and labels: launched by DbscanState::cluster_ids,
// labels_local and labels_global, and by the phased C-ABI bodies (the core-flag conversions,
// k_comp_out*).
// Reads parent, core, skey, sorig (or the inverse permutation in slab), rep, mutual, the cell
// records and the sorted points.  Writes cell_root, the component minima (ccmin, or cell_min per
// occupied cell on the per-cell path), min_bits / min_pref (MinRank; the cluster count at
// n_clusters_ptr()), the non-core queue (nc_list, its count at nc_list[n]) and the caller's
// labels.  Reads stdbscan_shared.inc and, from K6 (stdbscan_union.inc), the union-find helpers
// (uf_*).  The A/B-only forms (stdbscan_ab.inc) are included after k_label.
// Cluster id = rank of the component minimum among all minima (MinRank); core: own id; non-core:
// min id over adjacent core points, else -1.
//   local, per-cell path (cell_comp): k_cell_comp, k_word_popc, scan, k_near_bits (near_bits from
//     K6's core_bits, DbscanState::near_bits_ok), k_label_core_cells
//   local, otherwise: k_cell_roots, k_ccmin, k_word_popc, scan, k_label_core(_orig)
//   then k_label over the queued non-core points
//   global: k_cell_roots, k_ccmin_global, k_label_global_orig, k_label_global_core, k_label
//   phased: k_core_to_orig, k_core_from_orig, k_comp_out, k_comp_out_edges

__global__ __launch_bounds__(kBlock) void k_fill_i32(int32_t* p, int64_t n, int32_t v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// Cluster id of a component minimum m = its rank among the minima: one bit per original index
// (set by k_ccmin) and an exclusive scan of the words' popcounts (total = cluster count at
// pref[words]): n/32 words to clear and scan instead of an n-length flag array.
struct MinRank {
  const uint32_t* bits;
  const int32_t* pref;
  __device__ __forceinline__ int32_t operator[](int32_t m) const {
    const uint32_t w = bits[m >> 5];
    return pref[m >> 5] + __popc(w & ((1u << (m & 31)) - 1u));
  }
};

__global__ void k_word_popc(const uint32_t* __restrict__ bits, int64_t words,
                            int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = __popc(bits[i]);
}

// ccmin[s] = component-min original index for core points, -1 otherwise; flags the minima and
// queues the non-core points for k_label.
// Root of every occupied mutual cell's core points (its representative's root): the core points
// of a mutual cell all hang under the representative (star init), so k_ccmin takes their root
// from here -- one cached per-cell read instead of a parent chain per point.
__global__ __launch_bounds__(kBlock) void k_cell_roots(int32_t* parent,
                                                      const int32_t* __restrict__ occ,
                                                      const int32_t* __restrict__ n_occ,
                                                      int64_t cells,
                                                      const uint8_t* __restrict__ mutual,
                                                      const int32_t* __restrict__ rep,
                                                      int32_t* __restrict__ cell_root,
                                                      int32_t* __restrict__ zero = nullptr,
                                                      uint32_t* __restrict__ zwords = nullptr,
                                                      int64_t nzw = 0,
                                                      int32_t* __restrict__ cmin_fill = nullptr) {
  // zero (nullable): a counter of the next kernel, cleared here instead of by a memset launch;
  // likewise the label pass's minimum bits (zwords, nzw words) and its per-cell smallest keys
  // (cmin_fill: every cell INT_MAX) -- both first written by k_ccmin / k_ccmin_global next
  if (zero && blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;
  {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ts = (int64_t)gridDim.x * blockDim.x;
    if (zwords)
      for (int64_t i = t0; i < nzw; i += ts) zwords[i] = 0u;
    if (cmin_fill)
      for (int64_t i = t0; i < cells; i += ts) cmin_fill[i] = INT_MAX;
  }
  const int64_t m = *n_occ;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = occ[q];
    if ((int64_t)c >= cells) continue;
    const int r = mutual[c] ? rep[c] : -1;
    cell_root[c] = (r >= 0) ? uf_find(parent, r) : -1;  // -1: walk each point's own chain
  }
}

// cell_root (nullable): k_cell_roots' output (-1: not a mutual cell with core points), read for
// core points through skey.
// cell_key (nullable, pre-filled with INT_MAX): per cell the smallest component key among its
// core points, by a segmented wave minimum over the sorted points (k_cell_min_key fused in).
// The kItems points of a thread go through the dependent loads level by level (keys + flags,
// cell roots, component minima), each level's loads in flight together; the atomics come last.
__global__ __launch_bounds__(kBlock) void k_ccmin(int32_t* parent,
                                                 const uint8_t* __restrict__ core, int64_t n,
                                                 const int32_t* __restrict__ sorig,
                                                 int32_t* __restrict__ ccmin,
                                                 uint32_t* __restrict__ min_bits,
                                                 int32_t* __restrict__ nc_list,
                                                 int32_t* __restrict__ nc_count,
                                                 const int32_t* __restrict__ skey = nullptr,
                                                 const uint8_t* __restrict__ mutual = nullptr,
                                                 const int32_t* __restrict__ cell_root = nullptr,
                                                 int64_t cells = 0,
                                                 int32_t* __restrict__ cell_key = nullptr) {
  const int lane = threadIdx.x & 63;
  (void)mutual;
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < n;
       tile += (int64_t)gridDim.x * kBlock * kItems) {
    int32_t key[kItems], x[kItems];
    uint32_t cbits = 0, inb = 0;
#pragma unroll
    // levels 1, 2 and 4 load branch-free (clamped indices, results masked), so each level's
    // loads are in flight together; only the parent-chain walk (points outside mutual cells)
    // stays conditional
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      const int64_t sc = min(s, n - 1);
      const int32_t kv = skey ? skey[sc] : -1;  // kernel-uniform pointer test
      const uint8_t cv = core[sc];
      const bool in = s < n;
      key[k] = in ? kv : -1;
      inb |= in ? (1u << k) : 0u;
      cbits |= (in && cv) ? (1u << k) : 0u;
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      x[k] = -1;
      if (cell_root) {  // kernel-uniform
        const bool q = ((cbits >> k) & 1u) && key[k] >= 0 && (int64_t)key[k] < cells;
        const int32_t r = cell_root[q ? key[k] : 0];  // cells >= 1
        x[k] = q ? r : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int s = (int)(tile + (int64_t)k * kBlock + threadIdx.x);
      if (((cbits >> k) & 1u) && x[k] < 0) x[k] = uf_find(parent, s);
    }
    int m[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const bool c = (cbits >> k) & 1u;
      const int32_t v = sorig[c ? x[k] : 0];
      m[k] = c ? v : -1;
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      if ((inb >> k) & 1u) ccmin[s] = m[k];
      if (((cbits >> k) & 1u) && x[k] == (int)s) atomicOr(min_bits + (m[k] >> 5), 1u << (m[k] & 31));
    }
    if (cell_key) {  // kernel-uniform: every lane of the wave takes part
#pragma unroll
      for (int k = 0; k < kItems; ++k) {
        int v = (m[k] >= 0 && (int64_t)key[k] < cells) ? m[k] : INT_MAX;
        const int kk = key[k];
        // sorted keys: a run of equal keys is one cell; dist = lanes since this lane's run head
        const int prevk = __shfl_up(kk, 1, 64), next = __shfl_down(kk, 1, 64);
        const uint64_t hm = __ballot(lane == 0 || prevk != kk);
        const uint64_t upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
        const int dist = lane - (63 - __builtin_clzll(hm & upto));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int ov = __shfl_up(v, off, 64);
          if (off <= dist) v = min(v, ov);
        }
        if ((lane == 63 || next != kk) && kk >= 0 && v != INT_MAX) atomicMin(cell_key + kk, v);
      }
    }
    block_append_bits(tile, inb & ~cbits, nc_list, nc_count);
  }
}

// queue of the non-core points (phased / global labelling)
__global__ __launch_bounds__(kBlock) void k_nc_list(const uint8_t* __restrict__ core, int64_t n,
                                                   int32_t* __restrict__ nc_list,
                                                   int32_t* __restrict__ nc_count) {
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < n;
       tile += (int64_t)gridDim.x * kBlock * kItems)
    block_append(
        tile, n, [&](int64_t s) -> bool { return !core[s]; }, nc_list, nc_count);
}

// K7/K8 (core points): label = id of the component minimum
__global__ __launch_bounds__(kBlock) void k_label_core(const int32_t* __restrict__ ccmin,
                                                      int64_t n,
                                                      const int32_t* __restrict__ sorig,
                                                      MinRank cid,
                                                      int32_t* __restrict__ labels) {
  // kPU points per thread per tile, loads branch-free (clamped, masked): two memory rounds per
  // tile (ccmin + sorig, then the rank words) instead of two per point.  XCD-contiguous tiles
  // (grid a multiple of 8): the blocks of one XCD take one eighth of the sorted points, i.e. a
  // run of whole frames, so the labels they scatter (original order, within those frames) fill
  // their lines in that XCD's L2 instead of eight L2s writing partial lines of the same frames
  const int64_t T = (n + (int64_t)kBlock * kPU - 1) / ((int64_t)kBlock * kPU);
  const bool xm = (gridDim.x & 7) == 0;
  const int64_t xg = blockIdx.x & 7, nbx = gridDim.x >> 3;
  const int64_t t_lo = xm ? T * xg / 8 : blockIdx.x, t_hi = xm ? T * (xg + 1) / 8 : T;
  const int64_t t_step = xm ? nbx : gridDim.x;
  for (int64_t ti = t_lo + (xm ? (int64_t)(blockIdx.x >> 3) : 0); ti < t_hi; ti += t_step) {
    const int64_t tile = ti * kBlock * kPU;
    int32_t own[kPU], so[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int64_t s = min(tile + (int64_t)u * kBlock + threadIdx.x, n - 1);
      own[u] = ccmin[s];
      so[u] = sorig[s];
    }
    uint32_t w[kPU];
    int32_t pr[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int32_t m = own[u] >= 0 ? own[u] : 0;
      w[u] = cid.bits[m >> 5];
      pr[u] = cid.pref[m >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int64_t s = tile + (int64_t)u * kBlock + threadIdx.x;
      if (s < n && own[u] >= 0)
        labels[so[u]] = pr[u] + __popc(w[u] & ((1u << (own[u] & 31)) - 1u));
    }
  }
}

// The same in ORIGINAL order through the grid build's inverse permutation spos: the labels are
// written in whole lines and the component keys gathered (a frame's keys stay in L2) instead of
// 4-byte label writes scattered over each frame, whose partly written lines L2 evicts (dense
// share: 1.23 GB written for 0.25 GB of labels).  Non-core points are left to k_label.
__global__ __launch_bounds__(kBlock) void k_label_core_orig(const int32_t* __restrict__ ccmin,
                                                           int64_t n,
                                                           const int32_t* __restrict__ spos,
                                                           MinRank cid,
                                                           int32_t* __restrict__ labels) {
  const int64_t T = (n + (int64_t)kBlock * kPU - 1) / ((int64_t)kBlock * kPU);
  const bool xm = (gridDim.x & 7) == 0;  // XCD-contiguous tiles (runs of whole frames)
  const int64_t xg = blockIdx.x & 7, nbx = gridDim.x >> 3;
  const int64_t t_lo = xm ? T * xg / 8 : blockIdx.x, t_hi = xm ? T * (xg + 1) / 8 : T;
  const int64_t t_step = xm ? nbx : gridDim.x;
  for (int64_t ti = t_lo + (xm ? (int64_t)(blockIdx.x >> 3) : 0); ti < t_hi; ti += t_step) {
    const int64_t tile = ti * kBlock * kPU;
    int32_t sp[kPU], own[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u)  // branch-free (clamped); streamed once
      sp[u] = __builtin_nontemporal_load(spos + min(tile + (int64_t)u * kBlock + threadIdx.x,
                                                     n - 1));
#pragma unroll
    for (int u = 0; u < kPU; ++u) own[u] = ccmin[sp[u]];
    uint32_t w[kPU];
    int32_t pr[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int32_t m = own[u] >= 0 ? own[u] : 0;
      w[u] = cid.bits[m >> 5];
      pr[u] = cid.pref[m >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int64_t i = tile + (int64_t)u * kBlock + threadIdx.x;
      if (i < n && own[u] >= 0)
        labels[i] = pr[u] + __popc(w[u] & ((1u << (own[u] & 31)) - 1u));
    }
  }
}

// ---- component ids per CELL (all_mutual grids; after k_parent_init_cells and the union passes)
// Every occupied cell is mutual, so its core points share one component and the component
// minimum is a per-cell value: cell_key[c] = sorig[root(rep[c])] (cells without core points keep
// k_parent_init_cells' INT_MAX).  The cell whose representative is the root flags the minimum's
// bit.  Replaces k_cell_roots + k_ccmin: one thread per occupied cell instead of per point, and
// no per-point ccmin[] at all (k_label_core_cells reads cell_key through skey).
// zero: the non-core queue counter of k_label_core_cells (the union passes' list counter until
// here).
__global__ __launch_bounds__(kBlock) void k_cell_comp(int32_t* parent,
                                                     const int32_t* __restrict__ occ,
                                                     const int32_t* __restrict__ n_occ,
                                                     int64_t cells,
                                                     const int32_t* __restrict__ rep,
                                                     const int32_t* __restrict__ sorig,
                                                     int32_t* __restrict__ cell_key,
                                                     uint32_t* __restrict__ min_bits,
                                                     int32_t* __restrict__ zero) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;
  const int64_t m = *n_occ;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = occ[q];
    if ((int64_t)c >= cells) continue;
    const int r = rep[c];
    if (r < 0) continue;
    const int root = uf_find(parent, r);
    const int32_t k = sorig[root];
    cell_key[c] = k;
    if (root == r) atomicOr(min_bits + (k >> 5), 1u << (k & 31));
  }
}

// near_bits = core_bits dilated over the label pass's window (+-2 cells in x and y, +-rt slabs:
// slab_window's reach): one thread per word, every word written.  The key is (slab * ny + y) * nx
// + x, so a neighbour at (dx, dy, ds) is the bit at + (ds * ny + dy) * nx + dx: per (ds, dy) the
// three words around the shifted position give the five x shifts.  A shift that runs over a row or slab end only sets bits (the point is queued and finds no core cell); no
// true neighbour is lost, and words outside the array read as zero.  The bitmap stays in L2
// (0.86 MB at 1000 frames).
__global__ __launch_bounds__(kBlock) void k_near_bits(const uint32_t* __restrict__ core_bits,
                                                     int nbw, int nx, int ny, int rt,
                                                     uint32_t* __restrict__ near_bits) {
  // (the pass is VALU per word: 32-bit word indices -- the grid holds at most 2^30 cells -- and
  // one variable shift per row)
  auto word = [&](int k) -> uint32_t {  // branch-free: clamped index, result masked
    const uint32_t v = core_bits[min(max(k, 0), nbw - 1)];
    return (k >= 0 && k < nbw) ? v : 0u;
  };
  for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < nbw; w += gridDim.x * blockDim.x) {
    uint32_t acc = 0;
    for (int ds = -rt; ds <= rt; ++ds) {
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy) {
        // x = bits [p, p + 36) of the string: the row's cells x - 2 .. x + 2 of this word's 32
        const int64_t p = (int64_t)w * 32 + ((int64_t)ds * ny + dy) * nx - 2;
        const int k = (int)(p >> 5), sh = (int)(p & 31);  // (arithmetic shift: floor)
        const uint32_t a = word(k), b = word(k + 1), c = word(k + 2);
        uint64_t x = (((uint64_t)b << 32) | a) >> sh;
        x |= sh ? ((uint64_t)c << (64 - sh)) : 0ull;
        acc |= (uint32_t)(x | (x >> 1) | (x >> 2) | (x >> 3) | (x >> 4));
      }
    }
    near_bits[w] = acc;
  }
}

// K7/K8 (core points) on all_mutual grids, with the non-core queue folded in: a core point's
// label is the rank of its CELL's component minimum (cell_key[skey[s]]; sorted points are runs of
// equal keys, so the lookup is a broadcast load), a non-core point is queued for k_label.
// ORIG = false: over the sorted points, labels scattered through sorig (as k_label_core);
// ORIG = true : over the original indices through the inverse permutation spos (as
//               k_label_core_orig), the key and flag gathered, the queue entry = spos[i].
// kPU points per thread per tile, loads branch-free level by level, XCD-contiguous tiles (see
// k_label_core).
// guard: the box-certain union pass's count of non-mutual cells with core points.  all_mutual
// promises zero; if it is not, the labels are not valid and the cluster count (written by the
// scan before this kernel) is replaced by -1, which fails the call at the readback of the count.
// NEAR (near = k_near_bits' bitmap; null otherwise): a non-core point whose cell's bit is clear has no cell with a core
// point anywhere in its window, so its label is -1, written here, and it is not queued (on the
// radar stacks 43-46 % of the non-core points).  The word is loaded with cell_key[k], for the
// non-core points only: both depend on the key, so no level is added.  The isolated cell's points
// (key >= cells) stay queued.
struct AppendSpos {
  const int32_t* spos;
  __device__ int32_t operator()(int64_t i) const { return spos[i]; }
};
template <bool ORIG, bool NEAR>
__global__ __launch_bounds__(kBlock) void k_label_core_cells(
    const int32_t* __restrict__ skey, const uint8_t* __restrict__ core,
    const int32_t* __restrict__ perm, int64_t n, int64_t cells,
    const int32_t* __restrict__ cell_key, MinRank cid, int32_t* __restrict__ labels,
    int32_t* __restrict__ nc_list, int32_t* __restrict__ nc_count,
    const int32_t* __restrict__ guard, int32_t* __restrict__ n_clusters,
    const uint32_t* __restrict__ near) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && *guard != 0) *n_clusters = -1;
  const int64_t T = (n + (int64_t)kBlock * kPU - 1) / ((int64_t)kBlock * kPU);
  const bool xm = (gridDim.x & 7) == 0;
  const int64_t xg = blockIdx.x & 7, nbx = gridDim.x >> 3;
  const int64_t t_lo = xm ? T * xg / 8 : blockIdx.x, t_hi = xm ? T * (xg + 1) / 8 : T;
  const int64_t t_step = xm ? nbx : gridDim.x;
  for (int64_t ti = t_lo + (xm ? (int64_t)(blockIdx.x >> 3) : 0); ti < t_hi; ti += t_step) {
    const int64_t tile = ti * kBlock * kPU;
    int32_t pv[kPU], k[kPU];
    uint32_t c[kPU];
    if (ORIG) {
#pragma unroll
      for (int u = 0; u < kPU; ++u)  // streamed once
        pv[u] = __builtin_nontemporal_load(perm + min(tile + (int64_t)u * kBlock + threadIdx.x,
                                                       n - 1));
#pragma unroll
      for (int u = 0; u < kPU; ++u) {
        k[u] = skey[pv[u]];
        c[u] = core[pv[u]];
      }
    } else {
#pragma unroll
      for (int u = 0; u < kPU; ++u) {
        const int64_t s = min(tile + (int64_t)u * kBlock + threadIdx.x, n - 1);
        k[u] = skey[s];
        c[u] = core[s];
        pv[u] = perm[s];
      }
    }
    int32_t own[kPU];
    uint32_t inb = 0, cb = 0, far = 0;
    uint32_t nw[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {  // (non-core points only: a few per cent; no wait in here)
      const bool in = tile + (int64_t)u * kBlock + threadIdx.x < n;
      nw[u] = ~0u;
      if (NEAR && in && c[u] == 0u && k[u] >= 0 && (int64_t)k[u] < cells) nw[u] = near[k[u] >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const bool in = tile + (int64_t)u * kBlock + threadIdx.x < n;
      const bool q = in && c[u] != 0u && k[u] >= 0 && (int64_t)k[u] < cells;
      inb |= in ? (1u << u) : 0u;
      cb |= (in && c[u] != 0u) ? (1u << u) : 0u;
      const int32_t v = cell_key[q ? k[u] : 0];  // cells >= 1
      own[u] = (q && v != INT_MAX) ? v : -1;
    }
    if (NEAR) {
#pragma unroll
      for (int u = 0; u < kPU; ++u) far |= ((nw[u] >> (k[u] & 31)) & 1u) ? 0u : (1u << u);
    }
    uint32_t w[kPU];
    int32_t pr[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int32_t m = own[u] >= 0 ? own[u] : 0;
      w[u] = cid.bits[m >> 5];
      pr[u] = cid.pref[m >> 5];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      if (own[u] >= 0) {
        const int32_t lab = pr[u] + __popc(w[u] & ((1u << (own[u] & 31)) - 1u));
        if (ORIG)
          labels[tile + (int64_t)u * kBlock + threadIdx.x] = lab;
        else
          labels[pv[u]] = lab;
      } else if ((far >> u) & 1u) {
        if (ORIG)
          labels[tile + (int64_t)u * kBlock + threadIdx.x] = -1;
        else
          labels[pv[u]] = -1;
      }
    }
    if (ORIG)
      block_append_bits(tile, inb & ~cb & ~far, nc_list, nc_count, AppendSpos{perm});
    else
      block_append_bits(tile, inb & ~cb & ~far, nc_list, nc_count);
  }
}

// position of the n-th set bit of m (n < popcount(m)): halving by popcounts
__device__ __forceinline__ int nth_set_bit(uint64_t m, int n) {
  int pos = 0;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const int c = __popcll(m & ((1ull << s) - 1ull));
    if (n >= c) {
      n -= c;
      m >>= s;
      pos += s;
    }
  }
  return pos;
}

// K7/K8 (non-core points, queued): the smallest component key over adjacent core points, else
// none.  One wave per point, one lane per candidate cell of its window.  A cell whose box is
// wholly adjacent contributes its smallest key (cell_key) with no point read; the others are
// resolved in increasing cell_key order and only while that key can still beat the best so far:
// a mutual cell (one component) needs one adjacent core point, any other cell the smallest key
// among its adjacent core points.
// GLOBAL = false: key = ccmin (component-min original index, local run), label = cid[key];
// GLOBAL = true : key = slab (the core point's final label: labels are ranks of the sorted global
//                 representatives, so the smallest label is the smallest representative).
// ALLMUT (all_mutual grids, local run): every candidate cell with core points is mutual and key_of
//                 (ccmin) is not written -- the core flag core_of[j] stands for key_of[j] >= 0, the
//                 non-mutual search and the mutual[] loads compile out.
// XY: float2 points (ALLMUT grids only); the window comes from the key's slab.
// BITS (ALLMUT grids with integral-time windows, g.rt >= 0): the candidates are the set bits of
//                 core_bits in the window instead of a cell_key gather over all of it (below).
template <int D, bool GLOBAL, int W = 64, bool ALLMUT = false, bool XY = false, bool BITS = false>
// 6 waves/SIMD (80 VGPRs, no spill; with two candidate points per lane per round 7 spilled 8)
// W = 32: two points per wave, one per half (the same candidate loads per point, twice the
// points in flight: the pass is a chain of dependent loads per point, not bandwidth)
__global__ __launch_bounds__(kBlock, 6) void k_label(const Pt<XY>* __restrict__ pts,
                                                 const int32_t* __restrict__ skey, Geom g,
                                                 const CellRec<D>* __restrict__ crec,
                                                 const uint32_t* __restrict__ occ_bits,
                                                 const float2* __restrict__ slab_t,
                                                 const int32_t* __restrict__ key_of,
                                                 const int32_t* __restrict__ cell_key,
                                                 const uint8_t* __restrict__ mutual,
                                                 const int32_t* __restrict__ sorig,
                                                 MinRank cid,
                                                 const int32_t* __restrict__ nc_list,
                                                 const int32_t* __restrict__ nc_count,
                                                 int32_t* __restrict__ labels,
                                                 int32_t* __restrict__ kstat = nullptr,
                                                 const uint8_t* __restrict__ core_of = nullptr,
                                                 const uint32_t* __restrict__ core_bits = nullptr) {
  static_assert(!ALLMUT || (D == 2 && !GLOBAL), "all-mutual grids are 2-D, local runs");
  static_assert(!BITS || ALLMUT, "core_bits is built on the per-cell path of all-mutual grids");
  static_assert(!XY || ALLMUT, "xy points only on all-mutual grids");
  // kstat (A/B build, RPT_STATS): queued points, points with a core cell in their window, points
  // that searched a partly reachable cell, points labelled
  static_assert(W == 32 || W == 64, "a point per wave or per half-wave");
  constexpr int P = 64 / W;  // points per wave
  const int lane = threadIdx.x & 63;
  const int hl = lane & (W - 1);      // lane within the point's group
  const int h0 = lane - hl;           // the group's first lane
  const int shift = (W == 64) ? 0 : h0;
  // the group's bits of a wave ballot
  auto gbal = [&](bool v) -> uint64_t {
    const uint64_t b = __ballot(v);
    return (W == 64) ? b : ((b >> shift) & 0xffffffffull);
  };
  auto gmin = [&](int v) -> int {  // rows by DPP, then the 16 (and 32) lane steps
    v = row_reduce<16>(v, OpMin{});
    v = min(v, __shfl_xor(v, 16));
    if (W == 64) v = min(v, __shfl_xor(v, 32));
    return v;
  };
  const int64_t nc = *nc_count;
  // XCD-aware ranges of the (cell-ordered) queue: neighbouring points' windows share an L2
  const XcdRange xr = xcd_items((nc + P - 1) / P, true);
  for (int64_t qp = xr.first; qp < xr.end; qp += xr.step) {
    const int64_t q = qp * P + (lane / W);
    if (q >= nc) continue;  // (group-uniform)
    const int s = nc_list[q];
    const int32_t key = skey[s];
    int best = INT_MAX;
#ifdef RPT_AB
    bool st_core = false, st_search = false;
#endif
    if ((int64_t)key < g.cells) {
      const float4 p = load_pt<XY>(pts, s);
      int cx, cy, cz;
      decode_key<D>(key, g, cx, cy, cz);
      const Window w = XY ? slab_window<D>(cx, cy, cz, g.slab_of_key(key), g)
                          : make_window<D, false>(cx, cy, cz, p.w, p.w, g, slab_t);
      // super-rounds of kR candidates per lane, loads of one kind issued together: the cells'
      // smallest keys (empty cells hold INT_MAX, so no occupancy lookup), then the records of
      // the cells with core points -- two dependent rounds per super-round
      // BITS: the window's cells with core points come from core_bits first.  Each lane takes one
      // (slab, row) of the window (5 nS of them, W at a time) and reads the row's 5-bit field by a
      // two-word read; the five ballots of the field's bits are the set positions of this chunk
      // of rows, and the lanes take them one each (position idx = the idx-th set bit, x-major).
      // cell_key and the records are then loaded for cells with core points only (8-9 of the 75
      // on the radar stacks: one round), and cell_key needs no INT_MAX in the other cells.
      constexpr int NK = BITS ? 1 : kR;  // candidates per lane per super-round
      const int nrows = BITS ? 5 * w.nS : 1;
      for (int rbase = 0; rbase < nrows; rbase += W) {  // (one pass unless BITS; body not indented)
      uint64_t bx[5] = {0, 0, 0, 0, 0};
      int tot = w.total;
      if (BITS) {
        const int row = rbase + hl;
        const int ss = row / 5, yy = row - ss * 5;
        const int y = w.y0 + yy;
        uint32_t f = 0;
        if (row < nrows && y >= 0 && y < g.ny) {
          const int xlo = max(w.x0, 0), xhi = min(w.x0 + 4, g.nx - 1);  // (cx is in the grid)
          const int64_t pb = ((int64_t)(w.s0 + ss) * g.ny + y) * g.nx + xlo;
          const uint64_t two = ((uint64_t)core_bits[(pb >> 5) + 1] << 32) | core_bits[pb >> 5];
          f = ((uint32_t)(two >> (pb & 31)) & ((1u << (xhi - xlo + 1)) - 1u)) << (xlo - w.x0);
        }
        tot = 0;
#pragma unroll
        for (int xx = 0; xx < 5; ++xx) {
          bx[xx] = gbal((f >> xx) & 1u);
          tot += __popcll(bx[xx]);
        }
      }
      for (int base = 0; base < tot; base += W * NK) {
        int64_t c[NK];
        int ck[NK], cb[NK], ce[NK], cls[NK], mu[NK];
        if (BITS) {
          int idx = base + hl, qq = -1;
          if (idx < tot) {
            uint64_t m = 0;
            int xs = 0;
            bool found = false;
#pragma unroll
            for (int xx = 0; xx < 5; ++xx) {
              const int cn = __popcll(bx[xx]);
              if (!found && idx < cn) {
                m = bx[xx];
                xs = xx;
                found = true;
              }
              if (!found) idx -= cn;
            }
            qq = (rbase + nth_set_bit(m, idx)) * 5 + xs;
          }
          c[0] = (qq >= 0) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
        } else {
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int qq = base + k * W + hl;
            c[k] = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
          }
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) ck[k] = (c[k] >= 0) ? cell_key[c[k]] : INT_MAX;
        int v = INT_MAX;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          cb[k] = ce[k] = cls[k] = mu[k] = 0;
          if (ck[k] != INT_MAX) {
            const CellRec<D> cr = crec[c[k]];
            cb[k] = cr.b;
            ce[k] = cr.e;
            mu[k] = ALLMUT ? 1 : mutual[c[k]];
            cls[k] = classify<D, XY>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
            if (cls[k] == 1) v = min(v, ck[k]);
          }
        }
        best = min(best, gmin(v));
#ifdef RPT_AB
        {
          bool anyc = false;
#pragma unroll
          for (int k = 0; k < NK; ++k) anyc = anyc || ck[k] != INT_MAX;
          st_core = st_core || gbal(anyc) != 0;
        }
#endif
        // the partially reachable cells, smallest key first, while a key can still win
        uint32_t pend = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) pend |= (cls[k] == 2) ? (1u << k) : 0u;
        while (true) {
          int mine = INT_MAX, mk = -1;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (((pend >> k) & 1u) && ck[k] < best && ck[k] < mine) {
              mine = ck[k];
              mk = k;
            }
          const int mm = gmin(mine);
          if (mm == INT_MAX) break;
#ifdef RPT_AB
          st_search = true;
#endif
          const uint64_t at = gbal(mine == mm);
          const int l = h0 + __ffsll((unsigned long long)at) - 1;
          const int kl = __shfl(mk, l);
          int bsel = 0, esel = 0, msel = 0;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (k == kl) {
              bsel = cb[k];
              esel = ce[k];
              msel = mu[k];
            }
          if (lane == l) pend &= ~(1u << kl);
          const int bl = __shfl(bsel, l), el = __shfl(esel, l);
          // two points per lane per round (their loads issued together): a dense cell costs
          // half the dependent round trips
          if (ALLMUT || __shfl(msel, l)) {  // one component: a single adjacent core point decides
            bool hit = false;
            for (int j0 = bl; j0 < el && !hit; j0 += 2 * W) {
              const int j = j0 + hl, j2 = j + W;
              const bool v1 = j < el, v2 = j2 < el;
              int k1, k2;
              if (ALLMUT) {
                k1 = (v1 && core_of[j]) ? 0 : -1;
                k2 = (v2 && core_of[j2]) ? 0 : -1;
              } else {
                k1 = v1 ? key_of[j] : -1;
                k2 = v2 ? key_of[j2] : -1;
              }
              const float4 p1 = v1 ? load_pt<XY>(pts, j) : p;
              const float4 p2 = v2 ? load_pt<XY>(pts, j2) : p;
              hit = gbal((k1 >= 0 && adjacent<D, XY>(p, p1, g)) ||
                         (k2 >= 0 && adjacent<D, XY>(p, p2, g))) != 0;
            }
            if (hit) best = mm;
          } else {
            int lb = INT_MAX;
            for (int j0 = bl; j0 < el; j0 += 2 * W) {
              const int j = j0 + hl, j2 = j + W;
              const bool v1 = j < el, v2 = j2 < el;
              const int m1 = v1 ? key_of[j] : -1, m2 = v2 ? key_of[j2] : -1;
              const float4 p1 = v1 ? load_pt<XY>(pts, j) : p;
              const float4 p2 = v2 ? load_pt<XY>(pts, j2) : p;
              if (m1 >= 0 && m1 < best && m1 < lb && adjacent<D, XY>(p, p1, g)) lb = m1;
              if (m2 >= 0 && m2 < best && m2 < lb && adjacent<D, XY>(p, p2, g)) lb = m2;
            }
            best = min(best, gmin(lb));
          }
        }
      }
      }
    }
    if (hl == 0) {
      int32_t out = -1;
      if (best != INT_MAX) out = GLOBAL ? best : cid[best];
      labels[sorig[s]] = out;
#ifdef RPT_AB
      if (kstat) {
        atomicAdd(&kstat[0], 1);
        if (st_core) atomicAdd(&kstat[1], 1);
        if (st_search) atomicAdd(&kstat[2], 1);
        if (best != INT_MAX) atomicAdd(&kstat[3], 1);
      }
#endif
    }
  }
}

#ifdef RPT_AB
#include "stdbscan_ab.inc"
#endif

// Degenerate parameters (negative/NaN eps): nobody has a neighbour, not even itself.
__global__ __launch_bounds__(kBlock) void k_isolated_labels(int32_t* labels, int64_t n,
                                                           int singletons) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    labels[i] = singletons ? (int32_t)i : -1;
}

// Non-finite-time points are isolated; with min_samples <= 0 they are singleton clusters and
// flagged as their own component minimum (handled by k_ccmin via parent = self).

// ---------------------------------------------------------------- phased state (multi-GPU)
__global__ void k_core_to_orig(const uint8_t* __restrict__ core, const int32_t* __restrict__ sorig,
                               int64_t n, uint8_t* __restrict__ out) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    out[sorig[s]] = core[s];
}
__global__ void k_core_from_orig(const uint8_t* __restrict__ in, const int32_t* __restrict__ sorig,
                                 int64_t n, uint8_t* __restrict__ core) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    core[s] = in[sorig[s]] ? 1 : 0;
}
// comp[orig] = minimum original index of the point's core component, -1 for non-core; a core
// point of a mutual cell takes its cell's root (k_cell_roots: one load instead of a parent-chain
// walk per point)
__global__ void k_comp_out(int32_t* parent, const uint8_t* __restrict__ core,
                           const int32_t* __restrict__ sorig, int64_t n,
                           int32_t* __restrict__ comp, const int32_t* __restrict__ skey,
                           const int32_t* __restrict__ cell_root, int64_t cells) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    int32_t out = -1;
    if (core[s]) {
      const int32_t key = skey[s];
      const int32_t cr = ((int64_t)key < cells) ? cell_root[key] : -1;  // -1: not mutual
      out = sorig[cr >= 0 ? cr : uf_find(parent, (int)s)];
    }
    comp[sorig[s]] = out;
  }
}
// k_comp_out for the original indices outside [lo_end, hi_begin) only (the frame-sharded
// driver needs the component ids of its halo points and of its own edge points, not of the
// window's interior): every sorted point is read (one coalesced index load), only the edge
// points pay a root lookup and a scattered store
__global__ void k_comp_out_edges(int32_t* parent, const uint8_t* __restrict__ core,
                                 const int32_t* __restrict__ sorig, int64_t n,
                                 int32_t* __restrict__ comp, const int32_t* __restrict__ skey,
                                 const int32_t* __restrict__ cell_root, int64_t cells,
                                 int64_t lo_end, int64_t hi_begin) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = sorig[s];
    if (i >= lo_end && i < hi_begin) continue;
    int32_t out = -1;
    if (core[s]) {
      const int32_t key = skey[s];
      const int32_t cr = (cell_root && (int64_t)key < cells) ? cell_root[key] : -1;
      out = sorig[cr >= 0 ? cr : uf_find(parent, (int)s)];
    }
    comp[i] = out;
  }
}
// Global labelling, core points: ccmin[s] = component-min original index; each component's
// label = rank of its global representative (rep[min], from the equivalence merge) among the
// sorted representatives -- one binary search per component, at its root; non-core queued.
__global__ __launch_bounds__(kBlock) void k_ccmin_global(int32_t* parent,
                                                        const uint8_t* __restrict__ core,
                                                        int64_t n,
                                                        const int32_t* __restrict__ sorig,
                                                        const int64_t* __restrict__ rep,
                                                        const int64_t* __restrict__ reps,
                                                        int64_t nr, int32_t* __restrict__ ccmin,
                                                        int32_t* __restrict__ gl,
                                                        int32_t* __restrict__ nc_list,
                                                        int32_t* __restrict__ nc_count,
                                                        const int32_t* __restrict__ skey = nullptr,
                                                        const uint8_t* __restrict__ mutual = nullptr,
                                                        const int32_t* __restrict__ cell_root = nullptr,
                                                        int64_t cells = 0,
                                                        const int64_t* __restrict__ nr_dev = nullptr) {
  if (nr_dev) nr = *nr_dev;  // the representative count stays on the device (shard driver)
  // level by level as in k_ccmin (keys + flags, cell roots, originals: branch-free loads, each
  // level's loads in flight together); only the parent-chain walk stays conditional
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < n;
       tile += (int64_t)gridDim.x * kBlock * kItems) {
    int32_t key[kItems], x[kItems];
    uint32_t cbits = 0, nbits = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      const int64_t sc = min(s, n - 1);
      const int32_t kv = cell_root ? skey[sc] : -1;  // kernel-uniform pointer test
      const uint8_t cv = core[sc];
      const bool in = s < n;
      key[k] = in ? kv : -1;
      cbits |= (in && cv) ? (1u << k) : 0u;
      nbits |= (in && !cv) ? (1u << k) : 0u;  // non-core: queued for k_label
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      x[k] = -1;
      if (cell_root) {  // core points of a mutual cell: their cell's root (k_cell_roots)
        const bool q = ((cbits >> k) & 1u) && key[k] >= 0 && (int64_t)key[k] < cells;
        const int32_t kk = q ? key[k] : 0;  // cells >= 1
        const uint8_t mu = mutual[kk];
        const int32_t cr = cell_root[kk];
        x[k] = (q && mu) ? cr : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int s = (int)(tile + (int64_t)k * kBlock + threadIdx.x);
      if (((cbits >> k) & 1u) && x[k] < 0) x[k] = uf_find(parent, s);
    }
    int m[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const bool c = (cbits >> k) & 1u;
      const int32_t v = sorig[c ? x[k] : 0];
      m[k] = c ? v : -1;
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int64_t s = tile + (int64_t)k * kBlock + threadIdx.x;
      if ((cbits >> k) & 1u) {
        ccmin[s] = m[k];
        if (x[k] == (int)s) gl[m[k]] = rep_id(reps, nr, rep[m[k]]);
      }
    }
    block_append_bits(tile, nbits, nc_list, nc_count);
  }
}
// The core labels in original order through the grid build's inverse permutation (spos, the
// slab buffer before k_label_global_core reuses it): whole-line label writes (k_label_core_orig)
__global__ __launch_bounds__(kBlock) void k_label_global_orig(const uint8_t* __restrict__ core,
                                                             const int32_t* __restrict__ ccmin,
                                                             const int32_t* __restrict__ gl,
                                                             const int32_t* __restrict__ spos,
                                                             int64_t n,
                                                             int32_t* __restrict__ labels) {
  const int64_t T = (n + (int64_t)kBlock * kPU - 1) / ((int64_t)kBlock * kPU);
  for (int64_t ti = blockIdx.x; ti < T; ti += gridDim.x) {
    const int64_t tile = ti * kBlock * kPU;
    int32_t sp[kPU], m[kPU];
    uint8_t c[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u)  // branch-free (clamped)
      sp[u] = __builtin_nontemporal_load(spos + min(tile + (int64_t)u * kBlock + threadIdx.x,
                                                     n - 1));
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      c[u] = core[sp[u]];
      m[u] = ccmin[sp[u]];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int64_t i = tile + (int64_t)u * kBlock + threadIdx.x;
      if (i < n && c[u]) labels[i] = gl[m[u]];
    }
  }
}

// slab[s] = final label of core point s (-1 for non-core); core labels written out
// The core points' final labels (slab[s] = label, -1 for non-core) and, k_cell_min_key folded in,
// per cell the smallest label of its core points (cell_key pre-filled with INT_MAX): a segmented
// wave minimum over the sorted points, one atomic per cell run of a wave.
__global__ __launch_bounds__(kBlock) void k_label_global_core(const uint8_t* __restrict__ core,
                                                             const int32_t* __restrict__ ccmin,
                                                             const int32_t* __restrict__ gl,
                                                             const int32_t* __restrict__ sorig,
                                                             int64_t n,
                                                             int32_t* __restrict__ slab,
                                                             int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ skey,
                                                             int64_t cells,
                                                             int32_t* __restrict__ cell_key) {
  const int lane = threadIdx.x & 63;
  for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x; s0 < n;
       s0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = s0 + threadIdx.x;
    int32_t l = -1, key = -1;
    if (s < n) {
      key = skey[s];
      if (core[s]) {
        l = gl[ccmin[s]];
        if (labels) labels[sorig[s]] = l;  // (kernel-uniform; null: k_label_global_orig's)
      }
      slab[s] = l;
    }
    int v = (l >= 0 && (int64_t)key < cells) ? l : INT_MAX;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int ov = __shfl_up(v, off, 64);
      const int ok = __shfl_up(key, off, 64);
      if (lane >= off && ok == key) v = min(v, ov);
    }
    const int next = __shfl_down(key, 1, 64);
    if ((lane == 63 || next != key) && key >= 0 && v != INT_MAX) atomicMin(cell_key + key, v);
  }
}
