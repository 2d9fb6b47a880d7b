// K9 radix path: the kernels around radix_sort_pairs, launched by radix_front of summaries.hip in
// this order (the head kernel is the caller's: k_heads<FR> for summaries_impl, k_label_heads for
// label_means):
//   k_sum_keys      labels -> keys (label + 1, noise 0) and vals (point index)
//   (radix_sort_pairs: keys / vals -> sk / sv, stable, so each label's points stay in index order)
//   k_heads<FR>     sk, sv -> head[p] = 1 where a (label, frame) run of clustered points starts;
//                   first_noise[f] (nullable) = the first noise point of frame f.  Noise (key 0)
//                   sorts first in index order, so each frame's first noise point is the head of
//                   its frame within the noise run (no atomics)
//   k_label_heads   sk -> head[p] = 1 where a label run starts (no frames)
//   (exclusive_scan_total_i32: head -> pos, pos[n] = the run count, which stays on the device)
//   k_seg_starts    head, pos -> seg_start[run] = its first sorted position
//   k_gather_runs<VT>  sv, x, y, inten -> gx, gy, gi: the points of every run contiguous
// head is dead after k_seg_starts (summaries_impl reuses it as the long-run list).
// Reads summaries_shared.inc (FramesPf / FramesOff through FR).

__global__ void k_sum_keys(const int32_t* __restrict__ labels, int64_t n,
                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = (uint32_t)(labels[i] + 1);  // noise (-1) -> 0, sorts first
    vals[i] = (uint32_t)i;
  }
}

// head[p] = 1 where a (label, frame) run starts among clustered points; for the noise run, the
// first noise point of each frame is recorded.
template <class FR>
__global__ void k_heads(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                        FR fr, int64_t n, int32_t* __restrict__ head,
                        int64_t* __restrict__ first_noise) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = sk[p], i = sv[p];
    const int32_t f = fr.frame(i);
    const bool h = (p == 0) || k != sk[p - 1] || f != fr.frame(sv[p - 1]);
    head[p] = (k != 0u && h) ? 1 : 0;
    if (k == 0u && h && first_noise) first_noise[f] = (int64_t)i;
  }
}

// head[p] = 1 where a label run starts among clustered points (noise, key 0, excluded)
__global__ void k_label_heads(const uint32_t* __restrict__ sk, int64_t n,
                              int32_t* __restrict__ head) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = sk[p];
    head[p] = (k != 0u && (p == 0 || k != sk[p - 1])) ? 1 : 0;
  }
}

__global__ void k_seg_starts(const int32_t* __restrict__ head, const int32_t* __restrict__ pos,
                             int64_t n, int64_t* __restrict__ seg_start) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x)
    if (head[p]) seg_start[pos[p]] = p;
}

// points of every run gathered contiguously (coalesced writes, one gather read per point)
template <class VT>
__global__ void k_gather_runs(const uint32_t* __restrict__ sv, int64_t n,
                              const float* __restrict__ x, const float* __restrict__ y,
                              const VT* __restrict__ inten, float* __restrict__ gx,
                              float* __restrict__ gy, VT* __restrict__ gi) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t i = sv[p];
    gx[p] = x[i];
    gy[p] = y[i];
    gi[p] = inten[i];
  }
}
