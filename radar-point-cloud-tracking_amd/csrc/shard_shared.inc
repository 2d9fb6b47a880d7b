// Frame-sharded driver (shard.cpp), what more than one stage file or the driver reads; no kernel
// is here.  kHaloHdr: the header words of a halo buffer (k_halo_pack writes them, k_window and
// k_window_halo read them, halo_total decodes the owner's kept total).  kMergeMax: the ids one
// workgroup merges in LDS (k_merge_pairs; the driver sizes keys / vals by it).  WinIds: window
// index -> global point id (k_comp_send, k_pairs, the representative kernels).  WinMeta: the
// window's counts, written by the window kernels and read back by rpt_shard_window.  lookup: the
// merge table's class minimum of an id (k_root_reps).

constexpr int kHaloHdr = 4;                       // int32 header words of a halo buffer
constexpr int kMergeMax = 8192;                   // ids merged in LDS by one workgroup

// window index -> global point id: [prev halo | own | next halo]
struct WinIds {
  int32_t rank;
  int64_t n_prev, n_own, k_prev_total;
  __device__ __host__ int64_t gid(int64_t c) const {
    if (c < n_prev) return ((int64_t)(rank - 1) << kGidShift) | (k_prev_total - n_prev + c);
    if (c < n_prev + n_own) return ((int64_t)rank << kGidShift) | (c - n_prev);
    return ((int64_t)(rank + 1) << kGidShift) | (c - n_prev - n_own);
  }
};

struct WinMeta {  // device, one per step: read back with the window bounds
  int64_t n_prev, n_own, n_next, k_prev_total, n_head, n_tail, n_window, pad;
};

__device__ __forceinline__ int64_t halo_total(const int32_t* h) {
  return (int64_t)(((uint64_t)(uint32_t)h[2] << 32) | (uint64_t)(uint32_t)h[1]);
}

__device__ __forceinline__ int64_t lookup(const int64_t* __restrict__ keys,
                                          const int64_t* __restrict__ vals, int64_t m, int64_t v) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (lo < m && keys[lo] == v) ? vals[lo] : v;
}
