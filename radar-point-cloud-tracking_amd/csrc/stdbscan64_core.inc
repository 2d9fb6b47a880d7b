// stdbscan64.hip, the core flags.  Reads stdbscan64_shared.inc and the grid build's arrays.
// Leaves behind core[s] (sorted order): 1 where the point has at least min_samples neighbours,
// itself included.

// A group of kLanes lanes per point counts the point's neighbours range by range and stops at
// the first range after which the group's count has reached min_samples.  A point of the
// isolated cell has no neighbour, so its count is 0.
template <int D, bool TF64>
__global__ __launch_bounds__(kBlock) void k64_core(Pts64 p, Geom64 g,
                                                  const int32_t* __restrict__ cell_start,
                                                  const int32_t* __restrict__ skey, int32_t n,
                                                  uint8_t* __restrict__ core) {
  const int sub = threadIdx.x % kLanes;
  const int64_t gs = (int64_t)gridDim.x * kPtsPerBlock;
  for (int64_t s = (int64_t)blockIdx.x * kPtsPerBlock + threadIdx.x / kLanes; s < n; s += gs) {
    const int cell = skey[s];
    int cnt = 0, total = 0;
    if (cell < g.cells) {
      const P64 a = load_pt<D>(p, (int)s);
      walk64<D>(g, cell_start, cell, [&](int b, int e) {
        for (int j = b + sub; j < e; j += kLanes) cnt += near64<D, TF64>(a, load_pt<D>(p, j), g);
        total = group_sum(cnt);
        return total < g.min_samples;
      });
    }
    if (sub == 0) core[s] = total >= g.min_samples;
  }
}
