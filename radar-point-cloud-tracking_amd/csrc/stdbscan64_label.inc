// stdbscan64.hip, ids and labels.  Reads stdbscan64_shared.inc, the grid build's arrays, core[]
// and the union stage's parent[] (uf_root).  A cluster's id is the rank of its root among the
// roots in original order: roots are the components' minimum core indices, so ids ascend with
// them.

__global__ __launch_bounds__(kBlock) void k64_fill(int32_t* __restrict__ labels, int32_t n,
                                                  bool iota) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += ts)
    labels[i] = iota ? (int32_t)i : -1;
}

// is_root[o] (original order, every entry written): o is a core point and its component's root
__global__ __launch_bounds__(kBlock) void k64_roots(const int32_t* __restrict__ sorig,
                                                   const uint8_t* __restrict__ core,
                                                   const int32_t* __restrict__ parent, int32_t n,
                                                   int32_t* __restrict__ is_root) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += ts) {
    const int o = sorig[s];
    is_root[o] = (core[s] && parent[o] == o) ? 1 : 0;
  }
}

// cid[s] (sorted order): a core point's cluster id (rank: the exclusive scan of is_root), -1 for
// a non-core point
__global__ __launch_bounds__(kBlock) void k64_cid(const int32_t* __restrict__ sorig,
                                                 const uint8_t* __restrict__ core,
                                                 const int32_t* __restrict__ parent,
                                                 const int32_t* __restrict__ rank, int32_t n,
                                                 int32_t* __restrict__ cid) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < n; s += ts)
    cid[s] = core[s] ? rank[uf_root(parent, sorig[s])] : -1;
}

// A group of kLanes lanes per point: a core point takes its id, any other point the smallest id
// among its core neighbours (-1 when it has none, and for a non-core point of the isolated cell).
template <int D, bool TF64>
__global__ __launch_bounds__(kBlock) void k64_label(Pts64 p, Geom64 g,
                                                   const int32_t* __restrict__ cell_start,
                                                   const int32_t* __restrict__ skey,
                                                   const int32_t* __restrict__ sorig,
                                                   const int32_t* __restrict__ cid, int32_t n,
                                                   int32_t* __restrict__ labels) {
  const int sub = threadIdx.x % kLanes;
  const int64_t gs = (int64_t)gridDim.x * kPtsPerBlock;
  for (int64_t s = (int64_t)blockIdx.x * kPtsPerBlock + threadIdx.x / kLanes; s < n; s += gs) {
    const int cell = skey[s];
    int id = cid[s];
    if (id < 0 && cell < g.cells) {
      const P64 a = load_pt<D>(p, (int)s);
      int best = INT_MAX;
      walk64<D>(g, cell_start, cell, [&](int b, int e) {
        for (int j = b + sub; j < e; j += kLanes) {
          const int c = cid[j];
          if (c >= 0 && c < best && near64<D, TF64>(a, load_pt<D>(p, j), g)) best = c;
        }
        return true;
      });
      best = group_min(best);
      id = best == INT_MAX ? -1 : best;
    }
    if (sub == 0) labels[sorig[s]] = id;
  }
}
