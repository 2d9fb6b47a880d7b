// K1 write pass from staged entries, output slots to threads: launched by write_impl of polar.hip
// when the count pass staged entries and ab().k1_expand is on.  One pair per staging layout:
//   by rank            k_group_starts   reads the group prefix and file_offsets; leaves one
//                                       64-bit word per group (first output, entry phase,
//                                       unstaged flag: the format below) and the list of
//                                       unstaged emitting groups with its count
//                      k_expand_write   reads the group words and the by-rank entries; writes
//                                       the outputs of the staged groups
//   file-contiguous    k_file_staged    reads file_offsets (and the group prefix of a file that
//                                       overflows its region); leaves staged_out[f] and the same
//                                       list of unstaged groups
//                      k_expand_stream  reads file_offsets, staged_out and the file regions;
//                                       writes the staged outputs of every file
// Both write kernels read the rows' scale / cos / sin and the files' gains, write x, y, val
// (float or the u8 sample), gain and point frame below cap, and leave one xy-bounds partial per
// block when bpart is given.  The listed groups are then written by k_group_write_u8<.., LIST>
// (polar_write.inc) and the partials of both reduced by k_bounds_parts.
// Reads polar_shared.inc (phase_base, XyBounds, GroupMap) and k1_emit.h.

// ---- expand write: output slots to threads (staged groups), by-rank layout
// The wave-per-group write above walks 3 M groups of ~16 outputs each with a dependent
// prefix -> entry -> store chain per group; its time is that chain times the groups per wave
// slot.  Here the outputs themselves are spread over the threads: per group one 64-bit word
//   bits 0..39  gs    = global index of the group's first emitted output
//   bits 40..62 phase = slot position of that output's entry: its in-group kept rank
//               (first * stride - rank < stride), or its residue's base at stride 4
//   bit 63      the group emits outputs but is not staged (more than kStageSlots kept samples):
//               they are written by k_group_write_u8<.., LIST> over the list of such groups
// and a block walks a contiguous range of 1024-output tiles, finding each output's group by a
// binary search of an LDS window of those words (gs is non-decreasing in the group index).
constexpr int kGsBits = 40;
constexpr uint64_t kGsMask = (1ull << kGsBits) - 1ull;
constexpr uint64_t kUnstaged = 1ull << 63;
constexpr int kTileOut = 1024;  // outputs per block tile, 4 per thread (8: 86 VGPRs, slower)
constexpr int kOutPerThread = kTileOut / kBlock;
static_assert(kOutPerThread % 4 == 0, "k_expand_write stores a thread's outputs as 16-B vectors");
constexpr int kWin = 1024;  // groups in the LDS window

__global__ __launch_bounds__(kBlock) void k_group_starts(const int64_t* __restrict__ gprefix,
                                                        const int64_t* __restrict__ file_offsets,
                                                        uint32_t n_groups, uint32_t gpf,
                                                        uint32_t stride,
                                                        uint64_t* __restrict__ gword,
                                                        uint32_t* __restrict__ list,
                                                        uint32_t* __restrict__ list_n) {
  // the unstaged groups collect in a block LDS list over the whole grid-stride loop and go out
  // with ONE global atomic per block (one per block iteration was ~12 k same-address atomics per
  // 1000-frame stack, serialised in L2); a block whose list fills appends the rest directly
  constexpr uint32_t kCap = 2048;
  __shared__ uint32_t s_list[kCap];
  __shared__ uint32_t s_n, s_base;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  // power-of-two strides (the reference's 4) by shifts instead of divisions
  const EmitStride es = emit_stride(stride);
  for (uint32_t b0 = blockIdx.x * kBlock; b0 < n_groups; b0 += gridDim.x * kBlock) {
    const uint32_t g = b0 + threadIdx.x;
    if (g < n_groups) {
      const uint32_t f = g / gpf;
      const int64_t p0 = gprefix[g];
      // in-file rank and kept count: a file has fewer than 2^32 samples
      const uint32_t rank = (uint32_t)(p0 - gprefix[(int64_t)f * gpf]);
      const uint32_t total = (uint32_t)(gprefix[g + 1] - p0);
      const EmitSpan sp = emit_span(rank, total, es);
      const uint64_t gs = (uint64_t)file_offsets[f] + sp.first;
      // slot position of the first emitted output's entry: its in-group rank, or with stride 4
      // (residues packed, stage_pos) the base of its residue
      const uint64_t phase = stride == 4u ? (uint64_t)phase_base(sp.rank0, total)
                                          : (uint64_t)sp.rank0;
      const bool un = sp.m != 0u && total > (uint32_t)kStageSlots;
      gword[g] = gs | (phase << kGsBits) | (un ? kUnstaged : 0ull);
      if (un) {
        const uint32_t slot = atomicAdd(&s_n, 1u);
        if (slot < kCap)
          s_list[slot] = g;
        else
          list[atomicAdd(list_n, 1u)] = g;
      }
    }
  }
  __syncthreads();
  const uint32_t m = min(s_n, kCap);
  if (threadIdx.x == 0 && m) s_base = atomicAdd(list_n, m);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += kBlock) list[s_base + i] = s_list[i];
}

// largest g in [lo, hi) with gs(g) <= O, given gs(lo) <= O: one wave, 64-ary search
__device__ uint32_t wave_find_group(const uint64_t* __restrict__ gword, uint32_t lo, uint32_t hi,
                                    uint64_t O) {
  const uint32_t lane = threadIdx.x & 63u;
  while (hi - lo > 1u) {
    const uint32_t step = (hi - lo + 63u) / 64u;
    const uint32_t idx = lo + lane * step;
    const bool le = idx < hi && (gword[idx] & kGsMask) <= O;  // a prefix of the lanes
    const uint64_t m = __ballot(le);
    const uint32_t top = 63u - (uint32_t)__clzll((long long)m);
    lo = __builtin_amdgcn_readfirstlane(lo + top * step);
    hi = min(hi, lo + step);
  }
  return lo;
}

// same, one thread (the rare outputs beyond the LDS window)
__device__ uint32_t thread_find_group(const uint64_t* __restrict__ gword, uint32_t lo,
                                      uint32_t hi, uint64_t O) {
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if ((gword[mid] & kGsMask) <= O)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// largest j < wn with s_win[j].gs <= O (s_win[0].gs <= O)
__device__ __forceinline__ uint32_t lds_find(const uint64_t* s_win, uint32_t wn, uint64_t O) {
  uint32_t lo = 0u;
#pragma unroll
  for (uint32_t step = kWin / 2; step > 0u; step >>= 1)
    if (lo + step < wn && (s_win[lo + step] & kGsMask) <= O) lo += step;
  return lo;
}

// VEC: every output array is 16-B aligned (float4 / int4 stores of a thread's 4 outputs)
// VT: as k_group_write_u8's (uint8_t: a thread's four intensities are one 4-byte store)
template <bool VEC, class VT = float>
__global__ __launch_bounds__(kBlock) void k_expand_write(
    const uint64_t* __restrict__ gword, uint32_t n_groups, GroupMap gm, uint32_t estep,
    const float* __restrict__ scale, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, const int32_t* __restrict__ gain,
    const int64_t* __restrict__ total_out, int files_per_frame, float* __restrict__ x,
    float* __restrict__ y, VT* __restrict__ val, int32_t* __restrict__ gain_out,
    int32_t* __restrict__ pf_out, int64_t cap, const uint32_t* __restrict__ entries,
    uint32_t* __restrict__ bpart = nullptr) {
  // bpart (nullable): this block's xy-bounds partial of the outputs it writes (XyBounds)
  __shared__ uint64_t s_win[kWin];
  __shared__ uint32_t s_glo;
  const int64_t total = min(*total_out, cap);
  const int64_t n_tiles = (total + kTileOut - 1) / kTileOut;
  const int64_t t0 = n_tiles * blockIdx.x / gridDim.x;
  const int64_t t1 = n_tiles * (blockIdx.x + 1) / gridDim.x;
  if (t0 >= t1) {  // block-uniform
    if (bpart && threadIdx.x < 4)  // (no outputs: the identity)
      bpart[4 * blockIdx.x + threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xffffffffu;
    return;
  }
  if (threadIdx.x < 64) {
    const uint32_t g = wave_find_group(gword, 0u, n_groups, (uint64_t)t0 * kTileOut);
    if (threadIdx.x == 0) s_glo = g;
  }
  __syncthreads();
  // the window of the next tile is loaded into registers while this tile's entries, geometry and
  // stores are in flight (its first group is known once phase A has searched this window)
  constexpr int kWinPer = kWin / kBlock;
  uint64_t wv[kWinPer];
  auto load_win = [&](uint32_t glo_) {
    const uint32_t wn_ = min((uint32_t)kWin, n_groups - glo_);
#pragma unroll
    for (int q = 0; q < kWinPer; ++q) {
      const uint32_t j = threadIdx.x + q * kBlock;
      wv[q] = j < wn_ ? gword[glo_ + j] : ~0ull;
    }
  };
  auto store_win = [&]() {
#pragma unroll
    for (int q = 0; q < kWinPer; ++q) s_win[threadIdx.x + q * kBlock] = wv[q];
  };
  uint32_t glo = s_glo;
  XyBounds xb;
  load_win(glo);
  store_win();
  __syncthreads();
  const float inv_bins = 1.0f / 1024.0f;  // exact: step = scale / 1024 == scale * 2^-10
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t wn = min((uint32_t)kWin, n_groups - glo);
    const bool truncated = glo + wn < n_groups;
    const uint64_t O0 = (uint64_t)t * kTileOut;
    // phase A: this thread's kOutPerThread consecutive outputs: the first one's group by the LDS
    // search, the others by stepping over group starts (empty groups share their successor's)
    auto word = [&](uint32_t g) -> uint64_t {
      return (g - glo < wn) ? s_win[g - glo] : gword[g];
    };
    auto next_gs = [&](uint32_t g) -> uint64_t {
      return g + 1u < n_groups ? (word(g + 1u) & kGsMask) : ~0ull;
    };
    const uint64_t Ob = O0 + (uint64_t)threadIdx.x * kOutPerThread;
    uint32_t grp[kOutPerThread], idx[kOutPerThread];
    bool ok[kOutPerThread];
    if ((int64_t)Ob < total) {
      const uint32_t j = lds_find(s_win, wn, Ob);
      uint32_t g = (j == wn - 1u && truncated) ? thread_find_group(gword, glo + j, n_groups, Ob)
                                               : glo + j;
      uint64_t w = word(g), nx = next_gs(g);
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        const uint64_t O = Ob + k;
        const bool in = (int64_t)O < total;
        while (in && O >= nx) {
          ++g;
          w = word(g);
          nx = next_gs(g);
        }
        ok[k] = in && !(w & kUnstaged);
        grp[k] = g;
        // the entry's slot position, mod 2^32 like the 64-bit form (only staged groups use it:
        // idx < kStageSlots).  estep, the entries from one output to the next: 1 at stride 4
        // (residues packed), else the stride
        const uint32_t d = (uint32_t)O - (uint32_t)w;
        idx[k] = d * estep + (uint32_t)((w & ~kUnstaged) >> kGsBits);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        ok[k] = false;
        grp[k] = glo;
        idx[k] = 0u;
      }
    }
    // the next tile's first group (thread 0), before the window is rewritten
    if (threadIdx.x == 0 && t + 1 < t1) {
      const uint64_t On = O0 + kTileOut;
      const uint32_t j = lds_find(s_win, wn, On);
      s_glo = (j == wn - 1u && truncated) ? thread_find_group(gword, glo + j, n_groups, On)
                                          : glo + j;
    }
    __syncthreads();  // every search of this window done; s_glo of the next tile visible
    if (t + 1 < t1) {
      glo = s_glo;
      load_win(glo);
    }
    // phase B: the staged entries, then the rows' geometry, then the stores
    uint32_t ent[kOutPerThread];
    // every load unconditional (a slot that writes nothing reads entry 0 / its group's first
    // row) and masked by selects: conditional loads would each end in a full vmcnt wait
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      const uint32_t e = entries[ok[k] ? (int64_t)grp[k] * kStageSlots + idx[k] : 0];
      ent[k] = ok[k] ? e : 0u;
    }
    float sc[kOutPerThread], cc[kOutPerThread], ss[kOutPerThread];
    uint32_t fl[kOutPerThread], pfl[kOutPerThread];
    // one division per thread: its outputs' groups are grp[0] or a few after it (steps over
    // file / frame boundaries instead of dividing again)
    const uint32_t f0 = grp[0] / gm.gpf, r0 = grp[0] - f0 * gm.gpf;
    const uint32_t fpf = (uint32_t)files_per_frame, p0 = f0 / fpf, q0 = f0 - p0 * fpf;
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      uint32_t f = f0, r = r0 + (grp[k] - grp[0]);
      while (r >= gm.gpf) {
        r -= gm.gpf;
        ++f;
      }
      uint32_t pf = p0, q = q0 + (f - f0);
      while (q >= fpf) {
        q -= fpf;
        ++pf;
      }
      fl[k] = f;
      pfl[k] = pf;
      const int64_t row = (int64_t)f * gm.rows + (int64_t)r * kGroupRows + (ent[k] >> 18);
      sc[k] = scale[row];
      cc[k] = cos_t[row];
      ss[k] = sin_t[row];
    }
    float ox[kOutPerThread], oy[kOutPerThread], ov[kOutPerThread];
    int32_t og[kOutPerThread], op[kOutPerThread];
    bool all_ok = true;
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      const float rr = sc[k] * inv_bins * (float)((ent[k] >> 8) & 1023u);
      ox[k] = rr * cc[k];
      oy[k] = rr * ss[k];
      ov[k] = (float)(ent[k] & 0xffu);
      og[k] = gain ? gain[fl[k]] : 0;
      op[k] = (int32_t)pfl[k];
      all_ok = all_ok && ok[k];
      if (bpart && ok[k]) xb.add(ox[k], oy[k]);
    }
    if (VEC && all_ok) {  // 16-B stores (the common case)
#pragma unroll
      for (int h = 0; h < kOutPerThread; h += 4) {
        const uint64_t o = Ob + h;
        *reinterpret_cast<float4*>(x + o) = make_float4(ox[h], ox[h + 1], ox[h + 2], ox[h + 3]);
        *reinterpret_cast<float4*>(y + o) = make_float4(oy[h], oy[h + 1], oy[h + 2], oy[h + 3]);
        if constexpr (sizeof(VT) == 1)
          *reinterpret_cast<uint32_t*>(val + o) =
              (ent[h] & 0xffu) | ((ent[h + 1] & 0xffu) << 8) | ((ent[h + 2] & 0xffu) << 16) |
              ((ent[h + 3] & 0xffu) << 24);
        else
          *reinterpret_cast<float4*>(val + o) = make_float4(ov[h], ov[h + 1], ov[h + 2], ov[h + 3]);
        if (gain_out)
          *reinterpret_cast<int4*>(gain_out + o) = make_int4(og[h], og[h + 1], og[h + 2], og[h + 3]);
        if (pf_out)
          *reinterpret_cast<int4*>(pf_out + o) = make_int4(op[h], op[h + 1], op[h + 2], op[h + 3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        if (!ok[k]) continue;
        const uint64_t oo = Ob + k;
        x[oo] = ox[k];
        y[oo] = oy[k];
        val[oo] = (VT)(ent[k] & 0xffu);
        if (gain_out) gain_out[oo] = og[k];
        if (pf_out) pf_out[oo] = op[k];
      }
    }
    if (t + 1 < t1) store_win();
    __syncthreads();  // the next tile's window
  }
  if (bpart) xb.store_block(bpart, reinterpret_cast<uint32_t*>(s_win), 1);  // (window done)
}

// ---- streaming write: output slots to threads, file-contiguous layout
// Output o of file f is word o of the file's region of C = gpf * kStageSlots words when
// o < staged_out[f] (k1_emit.h emit_staged_out), and its global slot is file_offsets[f] + o: the
// write pass is a stream over the regions with no group words and no per-output search.
//
// k_file_staged, one wave per file: staged_out[f], from the file's output count alone when it
// is at most C (no group of the file is unstaged: file_offsets[f], [f + 1] and nothing else are
// read).  Else the wave walks the file's group prefix, 64 groups at a time, and appends the
// unstaged emitting groups to the list that k_group_write_u8<.., LIST> writes from the echo (one
// global atomic per overflowing file: the groups are counted first and listed in a second walk).
__global__ __launch_bounds__(kBlock) void k_file_staged(const int64_t* __restrict__ gprefix,
                                                       const int64_t* __restrict__ file_offsets,
                                                       uint32_t n_files, uint32_t gpf,
                                                       uint32_t stride,
                                                       uint32_t* __restrict__ staged_out,
                                                       uint32_t* __restrict__ list,
                                                       uint32_t* __restrict__ list_n) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t fcap = gpf * (uint32_t)kStageSlots;
  for (uint32_t f = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + threadIdx.x / 64);
       f < n_files; f += gridDim.x * kWavesPerBlock) {  // wave-uniform
    // a file has fewer than 2^32 samples, so fewer outputs
    const uint32_t count = (uint32_t)(file_offsets[f + 1] - file_offsets[f]);
    uint32_t so = count;
    if (count > fcap) {  // wave-uniform
      const EmitStride es = emit_stride(stride);
      const int64_t* gp = gprefix + (int64_t)f * gpf;
      const int64_t p00 = gp[0];
      auto unstaged = [&](uint32_t g, EmitSpan* sp) -> bool {
        if (g >= gpf) return false;
        const int64_t p0 = gp[g];
        // in-file rank and kept count: a file has fewer than 2^32 samples
        *sp = emit_span((uint32_t)(p0 - p00), (uint32_t)(gp[g + 1] - p0), es);
        return emit_unstaged_file(*sp, fcap);
      };
      uint32_t n_un = 0u;
      for (uint32_t g0 = 0u; g0 < gpf; g0 += 64u) {
        EmitSpan sp{};
        if (unstaged(g0 + lane, &sp)) {
          so = emit_staged_out(so, sp, fcap);
          ++n_un;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        so = min(so, (uint32_t)__shfl_xor((int)so, off));
        n_un += (uint32_t)__shfl_xor((int)n_un, off);
      }
      uint32_t base = 0u;
      if (lane == 0u) base = atomicAdd(list_n, n_un);
      base = __builtin_amdgcn_readfirstlane(base);
      for (uint32_t g0 = 0u; g0 < gpf; g0 += 64u) {
        EmitSpan sp{};
        const bool un = unstaged(g0 + lane, &sp);
        const uint64_t b = __ballot(un);
        if (un) list[base + (uint32_t)rank_in_mask(b)] = f * gpf + g0 + lane;
        base += (uint32_t)__popcll(b);
      }
    }
    if (lane == 0u) staged_out[f] = so;
  }
}

constexpr int kFWin = kBlock;  // file offsets in the LDS window: one per thread

// largest i in [lo, hi) with fo[i] <= O, given fo[lo] <= O: one wave, 64-ary search
__device__ uint32_t wave_find_file(const int64_t* __restrict__ fo, uint32_t lo, uint32_t hi,
                                   int64_t O) {
  const uint32_t lane = threadIdx.x & 63u;
  while (hi - lo > 1u) {
    const uint32_t step = (hi - lo + 63u) / 64u;
    const uint32_t idx = lo + lane * step;
    const bool le = idx < hi && fo[idx] <= O;  // a prefix of the lanes
    const uint64_t m = __ballot(le);
    const uint32_t top = 63u - (uint32_t)__clzll((long long)m);
    lo = __builtin_amdgcn_readfirstlane(lo + top * step);
    hi = min(hi, lo + step);
  }
  return lo;
}

// same, one thread (the rare outputs beyond the LDS window)
__device__ uint32_t thread_find_file(const int64_t* __restrict__ fo, uint32_t lo, uint32_t hi,
                                     int64_t O) {
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (fo[mid] <= O)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// largest j < wn with s_fo[j] <= O (s_fo[0] <= O)
__device__ __forceinline__ uint32_t lds_find_file(const int64_t* s_fo, uint32_t wn, int64_t O) {
  uint32_t lo = 0u;
#pragma unroll
  for (uint32_t step = kFWin / 2; step > 0u; step >>= 1)
    if (lo + step < wn && s_fo[lo + step] <= O) lo += step;
  return lo;
}

// k_expand_stream: a block walks a contiguous range of 1024-output tiles, 4 consecutive outputs
// per thread.  A thread finds the file of its first output by a binary search of an LDS window of
// file_offsets (n_files + 1 values, the last one the total, so an output below the total always
// has a file) and steps over file boundaries and empty files for the other three.
// VEC, VT, cap, bpart: as k_expand_write's.
template <bool VEC, class VT = float>
__global__ __launch_bounds__(kBlock) void k_expand_stream(
    const int64_t* __restrict__ file_offsets, uint32_t n_files,
    const uint32_t* __restrict__ staged_out, GroupMap gm, const float* __restrict__ scale,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int32_t* __restrict__ gain, int files_per_frame, float* __restrict__ x,
    float* __restrict__ y, VT* __restrict__ val, int32_t* __restrict__ gain_out,
    int32_t* __restrict__ pf_out, int64_t cap, const uint32_t* __restrict__ entries,
    uint32_t* __restrict__ bpart = nullptr) {
  __shared__ int64_t s_fo[kFWin];
  __shared__ uint32_t s_flo;
  const uint32_t n_off = n_files + 1u;  // values of file_offsets
  const int64_t total = min(file_offsets[n_files], cap);
  const int64_t n_tiles = (total + kTileOut - 1) / kTileOut;
  const int64_t t0 = n_tiles * blockIdx.x / gridDim.x;
  const int64_t t1 = n_tiles * (blockIdx.x + 1) / gridDim.x;
  if (t0 >= t1) {  // block-uniform
    if (bpart && threadIdx.x < 4)  // (no outputs: the identity)
      bpart[4 * blockIdx.x + threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xffffffffu;
    return;
  }
  if (threadIdx.x < 64) {
    const uint32_t f = wave_find_file(file_offsets, 0u, n_off, t0 * kTileOut);
    if (threadIdx.x == 0) s_flo = f;
  }
  __syncthreads();
  // the window of the next tile is loaded into a register while this tile's entries, geometry
  // and stores are in flight
  int64_t wv;
  auto load_win = [&](uint32_t flo_) {
    wv = threadIdx.x < min((uint32_t)kFWin, n_off - flo_) ? file_offsets[flo_ + threadIdx.x]
                                                          : INT64_MAX;
  };
  uint32_t flo = s_flo;
  XyBounds xb;
  load_win(flo);
  s_fo[threadIdx.x] = wv;
  __syncthreads();
  const uint32_t fcap = gm.gpf * (uint32_t)kStageSlots;  // words of a file's region
  const uint32_t fpf = (uint32_t)files_per_frame;
  const float inv_bins = 1.0f / 1024.0f;  // exact: step = scale / 1024 == scale * 2^-10
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t wn = min((uint32_t)kFWin, n_off - flo);
    const bool truncated = flo + wn < n_off;
    const int64_t O0 = t * kTileOut;
    auto off = [&](uint32_t i) -> int64_t {  // file_offsets[i], i <= n_files
      return (i - flo < wn) ? s_fo[i - flo] : file_offsets[i];
    };
    // phase A: the file and the in-file index of this thread's kOutPerThread consecutive outputs
    const int64_t Ob = O0 + (int64_t)threadIdx.x * kOutPerThread;
    uint32_t fl[kOutPerThread], oi[kOutPerThread];
    bool in[kOutPerThread];
    if (Ob < total) {
      const uint32_t j = lds_find_file(s_fo, wn, Ob);
      uint32_t f = (j == wn - 1u && truncated) ? thread_find_file(file_offsets, flo + j, n_off, Ob)
                                               : flo + j;
      int64_t base = off(f), nx = off(f + 1u);
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        const int64_t O = Ob + k;
        in[k] = O < total;
        while (in[k] && O >= nx) {  // (O < total = the last offset: f stays below n_files)
          ++f;
          base = nx;
          nx = off(f + 1u);
        }
        fl[k] = f;
        oi[k] = (uint32_t)(O - base);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        in[k] = false;
        fl[k] = flo;
        oi[k] = 0u;
      }
    }
    // the next tile's first file (thread 0), before the window is rewritten
    if (threadIdx.x == 0 && t + 1 < t1) {
      const int64_t On = O0 + kTileOut;
      const uint32_t j = lds_find_file(s_fo, wn, On);
      s_flo = (j == wn - 1u && truncated) ? thread_find_file(file_offsets, flo + j, n_off, On)
                                          : flo + j;
    }
    __syncthreads();  // every search of this window done; s_flo of the next tile visible
    if (t + 1 < t1) {
      flo = s_flo;
      load_win(flo);
    }
    // phase B: the staged entries and the files' staged counts, then the rows' geometry, then
    // the stores.  Every load unconditional and masked by selects (conditional loads would each
    // end in a full vmcnt wait): an output that is not written reads word 0 and, when it is
    // beyond the file's staged outputs but inside its region, a word that may never have been
    // written; either is dropped before its row field is used.
    uint32_t ent[kOutPerThread];
    bool ok[kOutPerThread];
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      const uint32_t so = staged_out[fl[k]];  // <= fcap
      const uint32_t e =
          entries[(in[k] && oi[k] < fcap) ? (int64_t)fl[k] * fcap + oi[k] : (int64_t)0];
      ok[k] = in[k] && oi[k] < so;
      ent[k] = ok[k] ? e : 0u;
    }
    float sc[kOutPerThread], cc[kOutPerThread], ss[kOutPerThread];
    uint32_t pfl[kOutPerThread];
    // one division per thread: its outputs' files are fl[0] or a few after it (steps over frame
    // boundaries; a long run of empty files divides again)
    uint32_t pf = fl[0] / fpf, q = fl[0] - pf * fpf;
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      if (k > 0) {
        q += fl[k] - fl[k - 1];
        if (q >= fpf) {
          if (q < 2u * fpf) {
            q -= fpf;
            ++pf;
          } else {
            const uint32_t d = q / fpf;
            pf += d;
            q -= d * fpf;
          }
        }
      }
      pfl[k] = pf;
      const int64_t row = (int64_t)fl[k] * gm.rows + (ent[k] >> 18);
      sc[k] = scale[row];
      cc[k] = cos_t[row];
      ss[k] = sin_t[row];
    }
    float ox[kOutPerThread], oy[kOutPerThread];
    int32_t og[kOutPerThread], op[kOutPerThread];
    bool all_ok = true;
#pragma unroll
    for (int k = 0; k < kOutPerThread; ++k) {
      const float rr = sc[k] * inv_bins * (float)((ent[k] >> 8) & 1023u);
      ox[k] = rr * cc[k];
      oy[k] = rr * ss[k];
      og[k] = gain ? gain[fl[k]] : 0;
      op[k] = (int32_t)pfl[k];
      all_ok = all_ok && ok[k];
      if (bpart && ok[k]) xb.add(ox[k], oy[k]);
    }
    if (VEC && all_ok) {  // 16-B stores (the common case)
#pragma unroll
      for (int h = 0; h < kOutPerThread; h += 4) {
        const int64_t o = Ob + h;
        *reinterpret_cast<float4*>(x + o) = make_float4(ox[h], ox[h + 1], ox[h + 2], ox[h + 3]);
        *reinterpret_cast<float4*>(y + o) = make_float4(oy[h], oy[h + 1], oy[h + 2], oy[h + 3]);
        if constexpr (sizeof(VT) == 1)
          *reinterpret_cast<uint32_t*>(val + o) =
              (ent[h] & 0xffu) | ((ent[h + 1] & 0xffu) << 8) | ((ent[h + 2] & 0xffu) << 16) |
              ((ent[h + 3] & 0xffu) << 24);
        else
          *reinterpret_cast<float4*>(val + o) =
              make_float4((float)(ent[h] & 0xffu), (float)(ent[h + 1] & 0xffu),
                          (float)(ent[h + 2] & 0xffu), (float)(ent[h + 3] & 0xffu));
        if (gain_out)
          *reinterpret_cast<int4*>(gain_out + o) = make_int4(og[h], og[h + 1], og[h + 2], og[h + 3]);
        if (pf_out)
          *reinterpret_cast<int4*>(pf_out + o) = make_int4(op[h], op[h + 1], op[h + 2], op[h + 3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kOutPerThread; ++k) {
        if (!ok[k]) continue;
        const int64_t oo = Ob + k;
        x[oo] = ox[k];
        y[oo] = oy[k];
        val[oo] = (VT)(ent[k] & 0xffu);
        if (gain_out) gain_out[oo] = og[k];
        if (pf_out) pf_out[oo] = op[k];
      }
    }
    if (t + 1 < t1) s_fo[threadIdx.x] = wv;
    __syncthreads();  // the next tile's window
  }
  if (bpart) xb.store_block(bpart, reinterpret_cast<uint32_t*>(s_fo), 1);  // (window done)
}
