// Shard driver, the equivalence merge on the device.  Reads shard_shared.inc (kMergeMax).
//   rpt_shard_finish  k_merge_pairs (one workgroup), when the gathered pairs are given: reads every
//                     rank's row, leaves keys (sorted ids), vals (class minima) and meta

// Union of every rank's equivalence pairs (the all-gathered rows [count | 2*count ids], rows of
// row_words int64): ONE workgroup, ids in LDS -- bitonic sort, distinct ids, min-hooking
// union-find -- so every rank derives the same (keys sorted, vals = class minimum).  meta[0] = the
// number of ids, or -1 when more than merge_max (<= kMergeMax) would be merged (the caller merges
// on the host; rpt_shard_set_merge_limit lowers merge_max so tests reach that path);
// meta[1] = 1 when some row holds more pairs than its capacity (the step is redone).
__global__ __launch_bounds__(1024) void k_merge_pairs(const int64_t* __restrict__ g, int world,
                                                      int64_t row_words, int merge_max,
                                                      int64_t* __restrict__ keys,
                                                      int64_t* __restrict__ vals,
                                                      int64_t* __restrict__ meta) {
  __shared__ int64_t ids[kMergeMax];
  __shared__ int32_t par[kMergeMax];
  __shared__ int32_t s_total, s_ovf, s_changed, s_m;
  __shared__ int32_t s_wsum[16];
  const int tid = threadIdx.x;
  const int64_t cap = (row_words - 1) / 2;
  if (tid == 0) {
    int64_t tot = 0;
    int ovf = 0;
    for (int q = 0; q < world; ++q) {
      const int64_t c = g[(int64_t)q * row_words];
      ovf |= c > cap ? 1 : 0;
      tot += c < cap ? c : cap;
    }
    s_total = 2 * tot > merge_max ? -1 : (int32_t)tot;
    s_ovf = ovf;
  }
  __syncthreads();
  const int total = s_total;
  if (total < 0) {
    if (tid == 0) {
      meta[0] = -1;
      meta[1] = s_ovf;
    }
    return;
  }
  const int nid = 2 * total;
  int n2 = 2;
  while (n2 < nid) n2 <<= 1;
  // load the ids row by row (rows are few: the owning row by a linear walk)
  for (int i = tid; i < n2; i += 1024) {
    int64_t v = INT64_MAX;
    if (i < nid) {
      int p = i >> 1, q = 0;
      for (;; ++q) {
        const int64_t c = g[(int64_t)q * row_words];
        const int cc = (int)(c < cap ? c : cap);
        if (p < cc) break;
        p -= cc;
      }
      v = g[(int64_t)q * row_words + 1 + 2 * p + (i & 1)];
    }
    ids[i] = v;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const int64_t a = ids[i], b = ids[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            ids[i] = b;
            ids[l] = a;
          }
        }
      }
      __syncthreads();
    }
  // distinct ids: a block scan of the run heads, then the survivors move down (in place: a
  // survivor's new position never exceeds its old one, and all reads finish before the writes)
  constexpr int kPer = kMergeMax / 1024;
  int64_t mine[kPer];
  int head[kPer];
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = tid * kPer + u;
    mine[u] = i < nid ? ids[i] : INT64_MAX;
    head[u] = (i < nid && (i == 0 || ids[i - 1] != mine[u])) ? 1 : 0;
    cnt += head[u];
  }
  // block exclusive scan of cnt
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if ((tid & 63) >= off) incl += v;
  }
  if ((tid & 63) == 63) s_wsum[tid >> 6] = incl;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int w = 0; w < 16; ++w) {
      const int v = s_wsum[w];
      s_wsum[w] = run;
      run += v;
    }
    s_m = run;
  }
  __syncthreads();
  int pos = s_wsum[tid >> 6] + incl - cnt;
#pragma unroll
  for (int u = 0; u < kPer; ++u)
    if (head[u]) ids[pos++] = mine[u];
  __syncthreads();
  const int m = s_m;
  for (int i = tid; i < m; i += 1024) par[i] = i;
  // the pairs as index pairs (each thread keeps its own)
  constexpr int kPairsPer = kMergeMax / 2 / 1024;
  int ia[kPairsPer], ib[kPairsPer];
  auto find_id = [&](int64_t v) {
    int lo = 0, hi = m;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
#pragma unroll
  for (int u = 0; u < kPairsPer; ++u) {
    const int p = tid + u * 1024;
    ia[u] = -1;
    ib[u] = -1;
    if (p < total) {
      int pp = p, q = 0;
      for (;; ++q) {
        const int64_t c = g[(int64_t)q * row_words];
        const int cc = (int)(c < cap ? c : cap);
        if (pp < cc) break;
        pp -= cc;
      }
      ia[u] = find_id(g[(int64_t)q * row_words + 1 + 2 * pp]);
      ib[u] = find_id(g[(int64_t)q * row_words + 2 + 2 * pp]);
    }
  }
  __syncthreads();
  auto root = [&](int a) {
    while (true) {
      const int p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (p == a) return a;
      a = p;
    }
  };
  for (int it = 0; it < 4 * kMergeMax; ++it) {
    __syncthreads();  // every thread has read the last round's s_changed
    if (tid == 0) s_changed = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPairsPer; ++u) {
      if (ia[u] < 0) continue;
      const int ra = root(ia[u]), rb = root(ib[u]);
      if (ra != rb) {
        atomicMin(&par[ra > rb ? ra : rb], ra < rb ? ra : rb);
        s_changed = 1;
      }
    }
    __syncthreads();
    for (int i = tid; i < m; i += 1024) par[i] = root(i);  // compress (values only decrease)
    __syncthreads();
    const int ch = s_changed;
    if (!ch) break;
  }
  __syncthreads();
  for (int i = tid; i < m; i += 1024) {
    keys[i] = ids[i];
    vals[i] = ids[root(i)];  // the class root is its smallest index = smallest id
  }
  if (tid == 0) {
    meta[0] = m;
    meta[1] = s_ovf;
  }
}
