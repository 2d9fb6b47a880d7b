// Shard driver, the cross-rank equivalences of one rank.  Reads shard_shared.inc (WinIds).
//   rpt_shard_link   k_comp_send: reads the window's component ids, leaves the own edge points'
//                    global component ids in the two send buffers
//   rpt_shard_pairs  k_pairs_init -> k_pairs (prev halo) -> k_pairs (next halo) -> k_store_count:
//                    read the halo points' component ids and their owners' ids, leave
//                    pairs = [count | (lo, hi) x min(count, cap)] for the all-gather

// own edge points' global component ids for the neighbours (-1: not core)
__global__ void k_comp_send(const int32_t* __restrict__ comp, WinIds w, int64_t n_head,
                            int64_t n_tail, int64_t* __restrict__ cp, int64_t* __restrict__ cn) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (cp)
    for (int64_t i = i0; i < n_head; i += step) {
      const int32_t c = comp[w.n_prev + i];
      cp[i] = c >= 0 ? w.gid(c) : -1;
    }
  if (cn)
    for (int64_t i = i0; i < n_tail; i += step) {
      const int32_t c = comp[w.n_prev + w.n_own - n_tail + i];
      cn[i] = c >= 0 ? w.gid(c) : -1;
    }
}

// equivalence pairs (my id of a halo point's component, its owner's), both core, distinct; a
// pair equal to the previous point's is skipped (runs of one component along the halo) and, while
// the pair fits a 64-bit key -- my component's window index (31 bits) and the owner's id as
// (rank - my rank + 2, own index < 2^30) -- every repeat of a pair (device hash set, 2x the halo
// size, so a probe always ends); any rest is merged all the same.  out[0] = the full count (may
// exceed cap: only cap pairs are stored, the caller grows cap and redoes the step).
__global__ void k_pairs(const int32_t* __restrict__ comp, int64_t c0, WinIds w,
                        const int64_t* __restrict__ owner, int64_t n, int64_t cap,
                        unsigned long long* __restrict__ count,
                        unsigned long long* __restrict__ set, uint64_t set_mask,
                        int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = comp[c0 + i];
    const int64_t b = owner[i];
    if (c < 0 || b < 0) continue;
    const int64_t a = w.gid(c);
    if (a == b) continue;
    if (i > 0 && comp[c0 + i - 1] == c && owner[i - 1] == b) continue;
    const int64_t rd = (b >> kGidShift) - w.rank + 2;
    const int64_t bi = b & ((int64_t(1) << kGidShift) - 1);
    if (set && rd >= 0 && rd < 8 && bi < (int64_t(1) << 30)) {
      const unsigned long long key = ((unsigned long long)(uint32_t)c << 33) |
                                     ((unsigned long long)rd << 30) | (unsigned long long)bi;
      uint64_t slot = (key * 0x9E3779B97F4A7C15ull) >> 20;
      bool dup = false;
      for (;; ++slot) {
        slot &= set_mask;
        const unsigned long long prev = atomicCAS(&set[slot], ~0ull, key);
        if (prev == ~0ull) break;
        if (prev == key) {
          dup = true;
          break;
        }
      }
      if (dup) continue;
    }
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned long long k = atomicAdd(count, 1ull);
    if ((int64_t)k < cap) {
      out[1 + 2 * k] = lo;
      out[2 + 2 * k] = hi;
    }
  }
}

// the pair count and the distinct-pair set (all ones = empty) of rpt_shard_pairs, in one launch
__global__ void k_pairs_init(unsigned long long* __restrict__ count,
                             unsigned long long* __restrict__ set, uint64_t size) {
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) *count = 0ull;
  for (uint64_t i = i0; i < size; i += (uint64_t)gridDim.x * blockDim.x) set[i] = ~0ull;
}

__global__ void k_store_count(const unsigned long long* __restrict__ count,
                              int64_t* __restrict__ out) {
  if (threadIdx.x == 0) out[0] = (int64_t)*count;
}
