// K9 per-frame counting sort (frame-major points), launched by summaries_impl of summaries.hip when
// a frame averages at most 64 k points (C == 1; larger frames: summaries_fsort_chunked.inc):
//   k_frame_sort<FR, VT>  one block per frame; reads labels, x, y, inten -> gx, gy, gi (each
//                         (frame, label) run contiguous, in index order), fstart[f], the
//                         frame-local lists tstart / tlen / tlabel at [fstart[f] + q], tfirst,
//                         nseg_f[f], first_noise[f], *overflow
//   (exclusive_scan_total_i32: nseg_f -> base, base[n_frames] = the segment count)
//   k_seg_compact         frame-local lists -> o_frame, o_label, o_count, o_first, seg_start
//                         (frame-major; tlen is dead afterwards: the long-run list)
//   k_seg_total_fix       *overflow -> segment count -1: the caller redoes K9 on the radix path
// Segments come frame-major (hash order inside a frame) from here, label-major from the radix
// sort (consumers bucket them by frame, tracker.cpp order_clusters).
// kFs*, FsLds, fs_hash / fs_insert / fs_find*, wave_group and k_seg_compact / k_seg_total_fix are
// read by summaries_fsort_chunked.inc too (the one stage file that reads another).
// Reads summaries_shared.inc (FR, wave_incl_scan).

// ---- per-frame counting sort (point_frame non-decreasing) ----------------------------------
// One 16-wave block per frame (8 waves: the frame's chunk chain per wave set the time at 125
// frames).  Each wave owns a contiguous part of the frame's points; the frame's
// clustered labels get LDS hash slots (at most kFsMaxKeys distinct labels per frame, else the
// frame reports an overflow and the caller redoes K9 on the radix path), counted per (wave, slot),
// scanned into frame-local offsets and per-wave cursors, and the points scattered stably — a
// (frame, label) run is then contiguous and in index order, as the radix path gives.  Noise is
// not scattered; each frame's first noise point is the first one of its lowest wave.
constexpr int kFsWaves = 16, kFsSlots = 1024, kFsMaxKeys = kFsSlots / 2;
constexpr int kFsSpt = kFsSlots / (kFsWaves * 64);  // scan slots per thread
static_assert(kFsSpt >= 1 && kFsSpt * kFsWaves * 64 == kFsSlots, "frame sort slot split");

struct FsLds {
  int keys[kFsSlots];               // label + 1 per slot, or -1
  uint32_t cnt[kFsWaves][kFsSlots]; // per-wave counts, then per-wave cursors
  int off[kFsSlots];                // run start (frame-local) per slot
  uint32_t wsum[2][kFsWaves];
  int fnoise[kFsWaves];
  int nkeys, overflow;
};

__device__ __forceinline__ uint32_t fs_hash(int v) {
  return ((uint32_t)v * 2654435761u) >> (32 - 10);
}

__device__ int fs_insert(FsLds& L, int v) {
  uint32_t s = fs_hash(v);
  for (int probe = 0; probe < kFsSlots; ++probe) {
    const int k = __atomic_load_n(&L.keys[s], __ATOMIC_RELAXED);
    if (k == v) return (int)s;
    if (k == -1) {
      const int old = atomicCAS(&L.keys[s], -1, v);
      if (old == -1) {
        if (atomicAdd(&L.nkeys, 1) >= kFsMaxKeys) L.overflow = 1;
        return (int)s;
      }
      if (old == v) return (int)s;
    }
    s = (s + 1) & (kFsSlots - 1);
  }
  L.overflow = 1;
  return -1;
}

__device__ __forceinline__ int fs_find_keys(const int* keys, int v) {
  uint32_t s = fs_hash(v);
  for (int probe = 0; probe < kFsSlots; ++probe) {
    const int k = keys[s];
    if (k == v) return (int)s;
    if (k == -1) return -1;
    s = (s + 1) & (kFsSlots - 1);
  }
  return -1;
}
__device__ __forceinline__ int fs_find(const FsLds& L, int v) { return fs_find_keys(L.keys, v); }

// Lanes with equal keys in this 64-point step: the lowest such lane (leader), the lane's rank
// among them and their number.  One ballot per distinct key, scalar loop.
__device__ __forceinline__ void wave_group(int v, bool valid, int lane, int& leader, int& rank,
                                           int& cnt) {
  uint64_t rem = __ballot(valid);
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  leader = -1;
  rank = 0;
  cnt = 0;
  while (rem) {
    const int l = __builtin_ctzll(rem);
    const int u = __builtin_amdgcn_readlane(v, l);
    const bool mine = valid && v == u;
    const uint64_t m = __ballot(mine);
    if (mine) {
      leader = l;
      rank = __popcll(m & lt);
      cnt = __popcll(m);
    }
    rem &= ~m;
  }
}

// Per segment q of the frame the frame-local lists at [lo + q] get the run's start position,
// length and label; tmp_first[start] gets the run's first point index.
template <class FR, class VT>
__global__ __launch_bounds__(kFsWaves * 64) void k_frame_sort(
    const int32_t* __restrict__ labels, FR fr, int64_t n,
    const float* __restrict__ x, const float* __restrict__ y, const VT* __restrict__ inten,
    float* __restrict__ gx, float* __restrict__ gy, VT* __restrict__ gi,
    int32_t* __restrict__ fstart, int32_t* __restrict__ tmp_start, int32_t* __restrict__ tmp_len,
    int32_t* __restrict__ tmp_label, int32_t* __restrict__ tmp_first,
    int32_t* __restrict__ nseg_f, int64_t* __restrict__ first_noise,
    int32_t* __restrict__ overflow) {
  __shared__ FsLds L;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lo = __builtin_amdgcn_readfirstlane(fr.begin(n, f));
  const int hi = __builtin_amdgcn_readfirstlane(fr.begin(n, f + 1));
  for (int s = tid; s < kFsSlots; s += kFsWaves * 64) {
    L.keys[s] = -1;
#pragma unroll
    for (int q = 0; q < kFsWaves; ++q) L.cnt[q][s] = 0u;
  }
  if (tid == 0) {
    L.nkeys = 0;
    L.overflow = 0;
    fstart[f] = lo;
  }
  __syncthreads();
  // this wave's chunks of 64 points
  const int nch = (hi - lo + 63) / 64, cpw = (nch + kFsWaves - 1) / kFsWaves;
  const int cb0 = w * cpw, cb1 = min(nch, cb0 + cpw);
  // pass 1: counts per (wave, slot), one LDS update per distinct label per step (its leader)
  int wfn = INT_MAX;
  constexpr int U1 = 8;
  for (int cb = cb0; cb < cb1; cb += U1) {
    int lab[U1];
#pragma unroll
    for (int u = 0; u < U1; ++u) {
      const int i = lo + (cb + u) * 64 + lane;
      lab[u] = (cb + u < cb1 && i < hi) ? labels[i] : -2;
    }
#pragma unroll
    for (int u = 0; u < U1; ++u) {
      const int v = lab[u] + 1;
      if (wfn == INT_MAX) {
        const uint64_t m0 = __ballot(v == 0);
        if (m0) wfn = lo + (cb + u) * 64 + __builtin_ctzll(m0);
      }
      const bool valid = v >= 1;
      int leader, rank, cm;
      wave_group(v, valid, lane, leader, rank, cm);
      if (valid && lane == leader) {
        const int s = fs_insert(L, v);
        if (s >= 0) L.cnt[w][s] += (uint32_t)cm;
      }
    }
  }
  if (lane == 0) L.fnoise[w] = wfn;
  __syncthreads();
  if (L.overflow) {
    if (tid == 0) {
      nseg_f[f] = 0;
      atomicExch(overflow, 1);
    }
    return;
  }
  if (tid == 0 && first_noise) {
    int m = INT_MAX;
#pragma unroll
    for (int q = 0; q < kFsWaves; ++q) m = min(m, L.fnoise[q]);
    if (m != INT_MAX) first_noise[f] = m;
  }
  // scan: kFsSpt consecutive slots per thread; run offsets and segment slots in slot order
  uint32_t tt[kFsSpt];
  uint32_t a = 0u, pcount = 0u;
#pragma unroll
  for (int j = 0; j < kFsSpt; ++j) {
    const int sj = kFsSpt * tid + j;
    uint32_t t = 0u;
#pragma unroll
    for (int q = 0; q < kFsWaves; ++q) t += L.cnt[q][sj];
    tt[j] = t;
    a += t;
    pcount += (t != 0u);
  }
  const uint32_t ia = wave_incl_scan(a, lane), ip = wave_incl_scan(pcount, lane);
  if (lane == 63) {
    L.wsum[0][w] = ia;
    L.wsum[1][w] = ip;
  }
  __syncthreads();
  uint32_t pa = 0, pp = 0, ta = 0, tp = 0;
#pragma unroll
  for (int q = 0; q < kFsWaves; ++q) {
    if (q < w) {
      pa += L.wsum[0][q];
      pp += L.wsum[1][q];
    }
    ta += L.wsum[0][q];
    tp += L.wsum[1][q];
  }
  const uint32_t eo = pa + ia - a, eq = pp + ip - pcount;
  auto emit = [&](int s, uint32_t t, uint32_t o, uint32_t q) {
    if (t == 0u) return;
    L.off[s] = (int)o;
    tmp_start[lo + q] = lo + (int)o;
    tmp_len[lo + q] = (int)t;
    tmp_label[lo + q] = L.keys[s] - 1;
    uint32_t run = o;
#pragma unroll
    for (int r = 0; r < kFsWaves; ++r) {
      const uint32_t c = L.cnt[r][s];
      L.cnt[r][s] = run;
      run += c;
    }
  };
  {
    uint32_t o = eo, q = eq;
#pragma unroll
    for (int j = 0; j < kFsSpt; ++j) {
      emit(kFsSpt * tid + j, tt[j], o, q);
      o += tt[j];
      q += (tt[j] != 0u);
    }
  }
  if (tid == 0) nseg_f[f] = (int)tp;
  (void)ta;
  __syncthreads();
  // pass 2: stable scatter through the per-wave cursors
  constexpr int U2 = 4;
  for (int cb = cb0; cb < cb1; cb += U2) {
    int lab[U2];
    float px[U2], py[U2], pv[U2];
#pragma unroll
    for (int u = 0; u < U2; ++u) {
      const int i = lo + (cb + u) * 64 + lane;
      const bool in = cb + u < cb1 && i < hi;
      lab[u] = in ? labels[i] : -2;
      px[u] = in ? x[i] : 0.f;
      py[u] = in ? y[i] : 0.f;
      pv[u] = in ? inten[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U2; ++u) {
      const int i = lo + (cb + u) * 64 + lane;
      const int v = lab[u] + 1;
      const bool valid = v >= 1;
      int leader, rank, cm;
      wave_group(v, valid, lane, leader, rank, cm);
      int base = 0;
      if (valid && lane == leader) {
        const int s = fs_find(L, v);
        base = (int)L.cnt[w][s];
        L.cnt[w][s] = (uint32_t)(base + cm);
        if (base == L.off[s]) tmp_first[lo + base] = i;
      }
      base = __shfl(base, leader < 0 ? lane : leader);
      if (valid) {
        const int p = lo + base + rank;
        gx[p] = px[u];
        gy[p] = py[u];
        gi[p] = pv[u];
      }
    }
  }
}

// Frame-local segment lists -> the global frame-major list (one wave per frame).
__global__ void k_seg_compact(int32_t F, const int32_t* __restrict__ fstart,
                              const int32_t* __restrict__ nseg_f, const int32_t* __restrict__ base,
                              const int32_t* __restrict__ tmp_start,
                              const int32_t* __restrict__ tmp_len,
                              const int32_t* __restrict__ tmp_label,
                              const int32_t* __restrict__ tmp_first, int32_t* __restrict__ o_frame,
                              int32_t* __restrict__ o_label, int64_t* __restrict__ o_count,
                              int64_t* __restrict__ o_first, int64_t* __restrict__ seg_start) {
  const int lane = threadIdx.x & 63;
  const int w0 = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const int nw = gridDim.x * (blockDim.x / 64);
  for (int f = w0; f < F; f += nw) {
    const int lo = fstart[f], m = nseg_f[f], b = base[f];
    for (int q = lane; q < m; q += 64) {
      const int s = tmp_start[lo + q];
      o_frame[b + q] = f;
      o_label[b + q] = tmp_label[lo + q];
      o_count[b + q] = tmp_len[lo + q];
      o_first[b + q] = tmp_first[s];
      seg_start[b + q] = s;
    }
  }
}

__global__ void k_seg_total_fix(const int32_t* __restrict__ overflow, int32_t* __restrict__ total) {
  if (threadIdx.x == 0 && *overflow) *total = -1;
}
