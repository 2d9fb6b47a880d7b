// K9 run summaries: centroid and mean intensity of every (frame, label) run, launched by
// summaries_impl of summaries.hip after either sort (META: the frame sort wrote o_frame / o_label /
// o_count / o_first already and runs are not adjacent; otherwise the radix path's runs tile
// [0, n) and the metadata comes from sk / sv):
//   k_runs_lane<META, FR, VT>  reads seg_start, *n_seg_dev, gx, gy, gi (and sk, sv, or o_count);
//                              runs of up to kLaneChainMax points one lane each -> o_cx, o_cy,
//                              o_mi (and the metadata); longer runs -> long_list / *n_long
//                              (zeroed beforehand)
//   k_summarize<META, FR, VT>  the listed long runs, two waves each -> the same outputs
// Reduction orders are numpy's, reproduced exactly:
//   centroid       = np.mean(pts (k,2) float32, axis=0): sequential float32 sum in point order
//                    starting from the first point, then one float32 division by k;
//   mean_intensity = np.mean(I (k,) float32): np.add.reduce over 8192-element buffer chunks,
//                    each chunk summed pairwise (numpy pairwise_sum: 8 accumulators up to 128
//                    elements, halving split above), chunks accumulated sequentially, then a
//                    float32 division by k.
// Runs of up to kLaneChainMax points: one lane per run (k_runs_lane: 64 runs' order-preserving
// float32 chains per add instruction); a longer run takes one wave for its x and y chains (lanes 0
// and 1, fed from LDS, so it costs ~k dependent adds of ~4.4 cycles, not k memory latencies) and
// one for its intensity.
// Reads summaries_shared.inc (kBlock, to_float, load4, FR).

// numpy pairwise_sum over a[b .. b+len) (as float32), iterative form of the recursion.  Only
// reached when intensities are not small non-negative integers, or their sum reaches 2^24 (see
// k_summarize).
template <class VT>
__device__ float pairwise_f32(const VT* __restrict__ a, int64_t b, int64_t len) {
  int64_t sb[40], sl[40];
  int st[40];
  float vs[40];
  int sp = 0, vp = 0;
  sb[0] = b;
  sl[0] = len;
  st[0] = 0;
  sp = 1;
  while (sp > 0) {
    const int64_t bb = sb[sp - 1], ll = sl[sp - 1];
    if (ll < 8) {
      float r = 0.f;  // numpy: res = 0.; res += a[i]
      for (int64_t i = 0; i < ll; ++i) r = r + to_float(a[bb + i]);
      --sp;
      vs[vp++] = r;
    } else if (ll <= 128) {
      float r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = to_float(a[bb + k]);
      int64_t i = 8;
      for (; i < ll - (ll % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = r[k] + to_float(a[bb + i + k]);
      }
      float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; i < ll; ++i) res = res + to_float(a[bb + i]);
      --sp;
      vs[vp++] = res;
    } else {
      int64_t n2 = ll / 2;
      n2 -= n2 % 8;
      if (st[sp - 1] == 0) {
        st[sp - 1] = 1;
        sb[sp] = bb;  // left half first
        sl[sp] = n2;
        st[sp] = 0;
        ++sp;
      } else if (st[sp - 1] == 1) {
        st[sp - 1] = 2;
        sb[sp] = bb + n2;
        sl[sp] = ll - n2;
        st[sp] = 0;
        ++sp;
      } else {
        const float right = vs[--vp];
        const float left = vs[--vp];
        --sp;
        vs[vp++] = left + right;
      }
    }
  }
  return vs[0];
}

// Order-preserving float32 sums of gx[b..e) and gy[b..e) (np.add.reduce from the first element),
// computed by ONE wave: lanes stage 1,024-element chunks of both in the wave's LDS slice (the next
// chunks' loads in flight meanwhile) and the chains run in lane 0 (x) and lane 1 (y) of the same
// instructions, each lane consuming 16-byte LDS reads of its own half issued a batch ahead: one
// dependent v_add_f32 (~4.4 cycles on gfx950, tools/microbench/chain.hip) per element advances
// both chains, so a run costs one SIMD's issue slots once, not twice (a packed x/y add would be
// no faster: 8.5 cycles).  Lane 0 returns the x sum, lane 1 the y sum (other lanes repeat them).
constexpr int kSeqChunk = 1024;
__device__ __forceinline__ float seq_sum(const float* __restrict__ gx,
                                         const float* __restrict__ gy, int b, int e, int lane,
                                         float* __restrict__ sbuf) {
  constexpr int kPre = kSeqChunk / 64, kChunk = kSeqChunk, V = 8;
  float pre[kPre], prey[kPre];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int t = 0; t < kPre; ++t) {
      const int idx = c0 + t * 64 + lane;
      pre[t] = (idx < e) ? gx[idx] : 0.f;
      prey[t] = (idx < e) ? gy[idx] : 0.f;
    }
  };
  float* __restrict__ sb = sbuf + (lane & 1) * kChunk;  // this lane's chain: x or y
  float acc = 0.f;
  load_chunk(b);
  for (int c0 = b; c0 < e; c0 += kChunk) {
#pragma unroll
    for (int t = 0; t < kPre; ++t) {
      sbuf[t * 64 + lane] = pre[t];
      sbuf[kChunk + t * 64 + lane] = prey[t];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (c0 + kChunk < e) load_chunk(c0 + kChunk);
    const int m = (e - c0 < kChunk) ? (e - c0) : kChunk;
    int i = 0;
    if (c0 == b) {  // start from the first element, then reach a 4-aligned position
      acc = sb[0];
      for (i = 1; i < 4 && i < m; ++i) acc = acc + sb[i];
    }
    const float4* sb4 = reinterpret_cast<const float4*>(sb);
    if (i == 0 && m == kChunk) {
      // a whole chunk (the bulk of a long run): two 32-element register windows in ping-pong,
      // each filled by ONE burst of 8 LDS reads issued a window ahead of its adds (bursts, not
      // four reads between every 16 adds: 1.70 -> 1.56 ms on the dense share's 490 k-point
      // chains, tools/microbench/chain_lds.hip, where 64-element windows measure the same; the
      // dependent add alone, register operands, costs 5.0 cycles there and this feed 7.6)
      constexpr int kW = 8, kNw = kChunk / (4 * kW);
      float4 wa[kW], wb[kW];
#pragma unroll
      for (int u = 0; u < kW; ++u) wa[u] = sb4[u];
#pragma unroll
      for (int w = 0; w < kNw; w += 2) {
#pragma unroll
        for (int u = 0; u < kW; ++u) wb[u] = sb4[(w + 1) * kW + u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kW; ++u) {
          acc = acc + wa[u].x;
          acc = acc + wa[u].y;
          acc = acc + wa[u].z;
          acc = acc + wa[u].w;
        }
        if (w + 2 < kNw) {
#pragma unroll
          for (int u = 0; u < kW; ++u) wa[u] = sb4[(w + 2) * kW + u];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kW; ++u) {
          acc = acc + wb[u].x;
          acc = acc + wb[u].y;
          acc = acc + wb[u].z;
          acc = acc + wb[u].w;
        }
      }
      i = kChunk;
    } else if (i + 8 * V <= m) {
      // ping-pong register batches: the next 4V elements are read from LDS while the chain
      // consumes the current ones (no register copies between batches)
      float4 pa[V], pb[V];
#pragma unroll
      for (int u = 0; u < V; ++u) pa[u] = sb4[i / 4 + u];
      while (true) {
#pragma unroll
        for (int u = 0; u < V; ++u) pb[u] = sb4[i / 4 + V + u];
        __builtin_amdgcn_sched_barrier(0);  // keep the next batch's reads ahead of the chain
#pragma unroll
        for (int u = 0; u < V; ++u) {
          acc = acc + pa[u].x;
          acc = acc + pa[u].y;
          acc = acc + pa[u].z;
          acc = acc + pa[u].w;
        }
        i += 4 * V;
        if (i + 8 * V > m) {
#pragma unroll
          for (int u = 0; u < V; ++u) {
            acc = acc + pb[u].x;
            acc = acc + pb[u].y;
            acc = acc + pb[u].z;
            acc = acc + pb[u].w;
          }
          i += 4 * V;
          break;
        }
#pragma unroll
        for (int u = 0; u < V; ++u) pa[u] = sb4[i / 4 + V + u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < V; ++u) {
          acc = acc + pb[u].x;
          acc = acc + pb[u].y;
          acc = acc + pb[u].z;
          acc = acc + pb[u].w;
        }
        i += 4 * V;
        if (i + 8 * V > m) {
#pragma unroll
          for (int u = 0; u < V; ++u) {
            acc = acc + pa[u].x;
            acc = acc + pa[u].y;
            acc = acc + pa[u].z;
            acc = acc + pa[u].w;
          }
          i += 4 * V;
          break;
        }
      }
    }
    for (; i < m; ++i) acc = acc + sb[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  return acc;
}

// Mean intensity of g[b..e) by one wave: when every intensity is a non-negative integer and the
// total stays below 2^24, every summation order is exact (integer lane sums), which equals
// numpy's pairwise result; otherwise numpy's chunked pairwise sum is evaluated by lane 0.
// 32 loads per lane in flight per round.
template <class VT>
__device__ __forceinline__ float mean_intensity(const VT* __restrict__ gi, int b, int e,
                                                int lane) {
  constexpr int kU = 32;
  if constexpr (sizeof(VT) == 1) {
    // u8 samples: numpy's 8192-element buffer chunks [b + 8192 c, ...) one after the other.  A
    // chunk's pairwise float32 sum is its integer sum (every partial sum of at most 8192 values
    // of at most 255 is an integer below 2^24, exact in float32 in any order), so the wave sums
    // each chunk as integers -- whole 4-byte words, 32 per lane in flight (byte loads kept a
    // quarter of the bytes in flight and made this wave the longer one of a run's two) -- and
    // adds the chunks' sums in order, as np.add.reduce does; below 2^24 in total that chain is
    // exact as well and the integer total is used.  gi's base is 4-byte aligned (scratch carve).
    constexpr int kChunk = 8192;
    static_assert(kChunk == 4 * 64 * kU, "one round of word loads covers a chunk");
    uint64_t isum = 0;
    float tot = 0.f;
    for (int cb = b; cb < e; cb += kChunk) {
      const int ce = min(e, cb + kChunk);
      const int wb = min(ce, (cb + 3) & ~3);  // whole words [wb, we), at most 3 bytes either side
      const int we = wb + ((ce - wb) & ~3);
      uint32_t cs = 0;
      if (cb + lane < wb) cs += gi[cb + lane];
      if (we + lane < ce) cs += gi[we + lane];
      const uint32_t* __restrict__ wp = reinterpret_cast<const uint32_t*>(gi + wb);
      const int nw = (we - wb) >> 2;
      uint32_t w[kU];
#pragma unroll
      for (int t = 0; t < kU; ++t) {
        const int q = t * 64 + lane;
        w[t] = q < nw ? wp[q] : 0u;
      }
#pragma unroll
      for (int t = 0; t < kU; ++t)
        cs += (w[t] & 0xffu) + ((w[t] >> 8) & 0xffu) + ((w[t] >> 16) & 0xffu) + (w[t] >> 24);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cs += __shfl_xor(cs, off);
      isum += cs;
      tot = tot + (float)cs;
    }
    const float fk8 = (float)(e - b);
    return isum < 16777216u ? (float)isum / fk8 : tot / fk8;
  }
  uint64_t isum = 0;
  bool small_int = true;
  for (int c0 = b; c0 < e; c0 += 64 * kU) {
    float v[kU];
#pragma unroll
    for (int t = 0; t < kU; ++t) {
      const int idx = c0 + t * 64 + lane;
      v[t] = idx < e ? to_float(gi[idx]) : 0.f;
    }
#pragma unroll
    for (int t = 0; t < kU; ++t) {
      small_int = small_int && (v[t] >= 0.f && v[t] == floorf(v[t]) && v[t] < 16777216.f);
      isum += (uint32_t)v[t];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) isum += __shfl_xor(isum, off);
  const bool all_int = __all(small_int);
  const int k = e - b;
  const float fk = (float)k;
  if (all_int && isum < 16777216u) return (float)isum / fk;
  float tot = 0.f;
  if (lane == 0)
    for (int64_t c = 0; c < k; c += 8192) {
      const int64_t len = (k - c < 8192) ? (k - c) : 8192;
      tot = tot + pairwise_f32(gi, b + c, len);
    }
  return tot / fk;
}

// Runs of at most kLaneChainMax points are summarised one LANE per run (k_runs_lane below);
// longer runs take a wave for both chains (seq_sum: a wave-wide chain issues one or two useful
// adds per wave instruction, and thousands of short runs made K9 VALU-issue and latency bound).
// A lane streams ~32 points per memory round trip, a wave's chain ~1,000 per 4 us: the lane form
// wins only for short runs (3,072 made the 125-frame stack's K9 slower: 143 us of lane chains).
constexpr int kLaneChainMax = 128;

// META: run [b, e) of segment su (o_count holds the lengths: runs are not adjacent, noise slots
// sit between frames); otherwise runs tile [0, n).
template <bool META>
__device__ __forceinline__ void run_bounds(const int64_t* __restrict__ seg_start,
                                           const int64_t* __restrict__ o_count, int64_t n_seg,
                                           int64_t n, int64_t su, int& b, int& e) {
  b = (int)seg_start[su];
  e = META ? (int)(b + o_count[su]) : (int)((su + 1 < n_seg) ? seg_start[su + 1] : n);
}

// One lane per run: lane l of wave w summarises run 64 w + l -- the x and y chains
// (sequentially from the first point, np.mean axis 0) and the intensity sum (exact integer sum,
// see mean_intensity; numpy's pairwise sum by the lane otherwise) in one pass over 16-B loads,
// kLq float4s of each column per block, all in flight together: 64 runs' chains advance per add
// instruction, and the loads in flight per lane bound it (a radar stack's runs are a few points
// each, plus one long run per frame).  Runs longer than kLaneChainMax are listed for k_summarize
// (long_list / *n_long, zeroed beforehand) instead.  Every lane takes part in the wave-level
// steps; lanes without a run of their own walk an empty range.
constexpr int kLq = 8;  // float4 loads per column per block (32 points)
template <bool META, class FR, class VT>
__global__ __launch_bounds__(kBlock, 2) void k_runs_lane(
    const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv,
    const int64_t* __restrict__ seg_start, const int32_t* __restrict__ n_seg_dev, int64_t n,
    const float* __restrict__ gx, const float* __restrict__ gy, const VT* __restrict__ gi,
    FR fr, int32_t* __restrict__ o_frame, int32_t* __restrict__ o_label,
    int64_t* __restrict__ o_count, int64_t* __restrict__ o_first, float* __restrict__ o_cx,
    float* __restrict__ o_cy, float* __restrict__ o_mi, int32_t* __restrict__ long_list,
    int32_t* __restrict__ n_long) {
  const int64_t n_seg = *n_seg_dev;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  const int64_t groups = (n_seg + 63) / 64;
  for (int64_t w = w0; w < groups; w += nw) {  // (wave-uniform)
    const int64_t su = w * 64 + lane;
    const bool valid = su < n_seg;
    int b = 0, e = 0;
    if (valid) run_bounds<META>(seg_start, o_count, n_seg, n, su, b, e);
    const bool lng = valid && e - b > kLaneChainMax;
    const uint64_t lm = __ballot(lng);
    if (lm) {
      int base = 0;
      if (lane == 0) base = atomicAdd(n_long, __popcll(lm));
      base = __shfl(base, 0);
      if (lng) long_list[base + __popcll(lm & ((1ull << lane) - 1ull))] = (int32_t)su;
    }
    const bool mine = valid && !lng;
    if (!mine) b = e = 0;
    float ax = 0.f, ay = 0.f;
    uint64_t isum = 0;
    bool small_int = true;
    auto ivisit = [&](float v, bool on) {
      const bool ok = v >= 0.f && v == floorf(v) && v < 16777216.f;
      small_int = small_int && (ok || !on);
      isum += on ? (uint64_t)(uint32_t)v : 0ull;
    };
    int i = b;
    if (i < e) {
      ax = gx[i];
      ay = gy[i];
      ivisit(to_float(gi[i]), true);
      ++i;
    }
    for (; i < e && (i & 3); ++i) {
      ax = ax + gx[i];
      ay = ay + gy[i];
      ivisit(to_float(gi[i]), true);
    }
    // whole float4s [i, i + 4 nq) in blocks of kLq per column; the block loop runs to the wave's
    // largest block count with branch-free loads (a lane past its own blocks re-reads a valid
    // block, the longest lane's if it has none) and selects instead of branches around the adds
    const int nq = (e - i) >> 2;
    const int nblk = nq / kLq;
    int nbmax = nblk;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nbmax = max(nbmax, __shfl_xor(nbmax, off));
    if (nbmax > 0) {
      const int lmax = __ffsll((unsigned long long)__ballot(nblk == nbmax)) - 1;
      const int i0 = nblk > 0 ? i : __shfl(i, lmax);
      const int last = nblk > 0 ? nblk - 1 : 0;
      const float4* __restrict__ px = reinterpret_cast<const float4*>(gx + i0);
      const float4* __restrict__ py = reinterpret_cast<const float4*>(gy + i0);
      const VT* __restrict__ pi = gi + i0;
      for (int k = 0; k < nbmax; ++k) {
        const int kk = min(k, last);
        float4 qx[kLq], qy[kLq], qi[kLq];
#pragma unroll
        for (int u = 0; u < kLq; ++u) {
          qx[u] = px[kk * kLq + u];
          qy[u] = py[kk * kLq + u];
          qi[u] = load4(pi, kk * kLq + u);
        }
        const bool on = k < nblk;
#pragma unroll
        for (int u = 0; u < kLq; ++u) {
          float tx = ax + qx[u].x, ty = ay + qy[u].x;
          tx = tx + qx[u].y;
          ty = ty + qy[u].y;
          tx = tx + qx[u].z;
          ty = ty + qy[u].z;
          tx = tx + qx[u].w;
          ty = ty + qy[u].w;
          ax = on ? tx : ax;
          ay = on ? ty : ay;
          ivisit(qi[u].x, on);
          ivisit(qi[u].y, on);
          ivisit(qi[u].z, on);
          ivisit(qi[u].w, on);
        }
      }
    }
    for (int q = nblk * kLq; q < nq; ++q) {
      const float4 vx = reinterpret_cast<const float4*>(gx + i)[q];
      const float4 vy = reinterpret_cast<const float4*>(gy + i)[q];
      const float4 vi = load4(gi + i, q);
      ax = ax + vx.x;
      ax = ax + vx.y;
      ax = ax + vx.z;
      ax = ax + vx.w;
      ay = ay + vy.x;
      ay = ay + vy.y;
      ay = ay + vy.z;
      ay = ay + vy.w;
      ivisit(vi.x, true);
      ivisit(vi.y, true);
      ivisit(vi.z, true);
      ivisit(vi.w, true);
    }
    for (i += 4 * nq; i < e; ++i) {
      ax = ax + gx[i];
      ay = ay + gy[i];
      ivisit(to_float(gi[i]), true);
    }
    if (mine) {
      const int k = e - b;
      const float fk = (float)k;
      o_cx[su] = ax / fk;
      o_cy[su] = ay / fk;
      float mi;
      if (small_int && isum < 16777216u) {
        mi = (float)isum / fk;
      } else {  // numpy's pairwise sum (k <= kLaneChainMax < 8192: one buffer chunk)
        float tot = 0.f;
        tot = tot + pairwise_f32(gi, b, k);
        mi = tot / fk;
      }
      o_mi[su] = mi;
      if (!META) {
        const uint32_t i0 = sv[b];
        o_frame[su] = fr.frame(i0);
        o_label[su] = (int32_t)sk[b] - 1;
        o_count[su] = k;
        o_first[su] = i0;
      }
    }
  }
}

// The runs longer than kLaneChainMax (k_runs_lane's list): two waves each, one for the mean
// intensity (lane-parallel) and one for the x and y chains (np.mean axis 0, sequential float32 in
// index order; seq_sum) -- pure dependent-add chains, so no other work sits in their instruction
// stream.  META: the frame sort already wrote frame/label/count/first; otherwise the metadata
// comes from the sorted keys (written by the intensity wave).
template <bool META, class FR, class VT>
// 2 waves/SIMD (up to 256 VGPRs: the x and y prefetch registers and the chain's two register
// windows; 4 waves spilled 17; a long run's waves are few, occupancy does not bound them)
// (the radix path's u8 form, left to itself, takes 200 VGPRs -- 2 waves -- where its float form
// takes 159: held to the float form's 3 waves, 168 VGPRs, no spill)
__global__ __launch_bounds__(kBlock, (!META && sizeof(VT) == 1) ? 3 : 2) void k_summarize(
    const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv,
    const int64_t* __restrict__ seg_start, const int32_t* __restrict__ n_seg_dev, int64_t n,
    const float* __restrict__ gx, const float* __restrict__ gy, const VT* __restrict__ gi,
    FR fr, int32_t* __restrict__ o_frame, int32_t* __restrict__ o_label,
    int64_t* __restrict__ o_count, int64_t* __restrict__ o_first, float* __restrict__ o_cx,
    float* __restrict__ o_cy, float* __restrict__ o_mi, const int32_t* __restrict__ long_list,
    const int32_t* __restrict__ n_long_dev) {
  __shared__ float s_buf[kBlock / 64][2 * kSeqChunk];
  const int64_t n_seg = *n_seg_dev;  // the segment count stays on the device (no readback)
  const int64_t n_long = *n_long_dev;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t w = w0; w < 2 * n_long; w += nw) {
    const int su = __builtin_amdgcn_readfirstlane(long_list[w >> 1]);
    const int comp = __builtin_amdgcn_readfirstlane((int)(w & 1));
    int b, e;
    run_bounds<META>(seg_start, o_count, n_seg, n, su, b, e);
    b = __builtin_amdgcn_readfirstlane(b);
    e = __builtin_amdgcn_readfirstlane(e);
    const int k = e - b;
    const float fk = (float)k;
    if (comp == 1) {
      const float mi = mean_intensity(gi, b, e, lane);
      if (lane == 0) {
        o_mi[su] = mi;
        if (!META) {
          const uint32_t i0 = sv[b];
          o_frame[su] = fr.frame(i0);
          o_label[su] = (int32_t)sk[b] - 1;
          o_count[su] = k;
          o_first[su] = i0;
        }
      }
      continue;
    }
    const float sum = seq_sum(gx, gy, b, e, lane, s_buf[threadIdx.x / 64]);
    if (lane < 2) (lane ? o_cy : o_cx)[su] = sum / fk;
  }
}
