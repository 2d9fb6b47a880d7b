// stdbscan64.hip, the core-core components.  Reads stdbscan64_shared.inc, the grid build's
// arrays and core[].  Leaves behind parent[] (by ORIGINAL index): a forest in which every core
// point's root is the minimum original index of its component's core points.

__global__ __launch_bounds__(kBlock) void k64_parent_init(int32_t* __restrict__ parent,
                                                         int32_t n) {
  const int64_t ts = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += ts)
    parent[i] = (int32_t)i;
}

__device__ __forceinline__ int uf_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Find with path halving.  A link always points from a larger index to a smaller one, so a
// stale read is an older ancestor and the chain is finite; the halving store writes an ancestor
// over an ancestor.
__device__ __forceinline__ int uf_find(int32_t* parent, int x) {
  while (true) {
    const int p = uf_load(parent + x);
    if (p == x) return x;
    const int gp = uf_load(parent + p);
    if (gp == p) return p;
    __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}
// the same walk without a store (after the union pass: the forest is final)
__device__ __forceinline__ int uf_root(const int32_t* __restrict__ parent, int x) {
  while (true) {
    const int p = parent[x];
    if (p == x) return x;
    x = p;
  }
}
// Lock-free union: the larger root is linked below the smaller by a compare-and-swap on the
// larger root's own entry; a lost race retries from the value that won.  No lane waits for
// another: every retry follows a link that some other lane has completed.
__device__ __forceinline__ void uf_unite(int32_t* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int tmp = a;
      a = b;
      b = tmp;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;
    a = old;
  }
}

// A group of kLanes lanes per core point s: every core neighbour j < s (sorted order) is united
// with s, so each adjacent core pair is united once, by its later point.
template <int D, bool TF64>
__global__ __launch_bounds__(kBlock) void k64_union(Pts64 p, Geom64 g,
                                                   const int32_t* __restrict__ cell_start,
                                                   const int32_t* __restrict__ skey,
                                                   const int32_t* __restrict__ sorig,
                                                   const uint8_t* __restrict__ core, int32_t n,
                                                   int32_t* parent) {
  const int sub = threadIdx.x % kLanes;
  const int64_t gs = (int64_t)gridDim.x * kPtsPerBlock;
  for (int64_t s = (int64_t)blockIdx.x * kPtsPerBlock + threadIdx.x / kLanes; s < n; s += gs) {
    const int cell = skey[s];
    if (cell >= g.cells || !core[s]) continue;
    const P64 a = load_pt<D>(p, (int)s);
    const int oa = sorig[s];
    walk64<D>(g, cell_start, cell, [&](int b, int e) {
      e = min(e, (int)s);
      for (int j = b + sub; j < e; j += kLanes)
        if (core[j] && near64<D, TF64>(a, load_pt<D>(p, j), g)) uf_unite(parent, oa, sorig[j]);
      return true;
    });
  }
}
