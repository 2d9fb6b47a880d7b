// K1 count pass on grouped u8 sweeps (1024 bins, 16-B aligned rows), launched by count_impl of
// polar.hip.  Reads the echo once.  Leaves one kept count per GROUP of kGroupRows rows (the driver
// scans them into the group prefix, n_files * gpf + 1 values, in row_prefix) and, when the caller
// gave an entries buffer, the staged kept samples as kept_entry() words in one of the two layouts
// of polar_shared.inc ("Staged kept samples"):
//   k_group_count_u8<HI, STAGE>      groups to waves in any order; STAGE: a group of 1 ..
//                                    kStageSlots kept samples stores all of them in its slot (by
//                                    rank), for k_group_starts + k_expand_write
//   k_group_count_u8_files<HI, W>    a file's groups in order by one workgroup of W waves; stores
//                                    only the emitted entries, file-contiguous, for k_file_staged
//                                    + k_expand_stream.  W from count_waves_per_file (its table)
//   k_file_counts_groups             reads the group prefix; leaves per file ceil(kept / stride)
//                                    (the driver scans them into file_offsets)
// A group that is not staged is read from the echo again by the write pass (polar_write.inc).
// Reads polar_shared.inc and k1_emit.h (emit_span, emit_staged_file, busiest_cu_files).

template <bool HI, bool STAGE>
__global__ __launch_bounds__(kBlock) void k_group_count_u8(const uint8_t* __restrict__ echo,
                                                          uint32_t n_groups, GroupMap gm,
                                                          uint32_t K,
                                                          int32_t* __restrict__ group_count,
                                                          uint32_t* __restrict__ entries,
                                                          int ph4) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock +
                                                        threadIdx.x / 64);
  const uint32_t n_waves = gridDim.x * kWavesPerBlock;
  // the group's (file, group-in-file) stepped incrementally: one division per wave, not one per
  // group (a 32-bit division by a runtime value is a few dozen scalar instructions)
  const uint32_t dq = n_waves / gm.gpf, dr = n_waves - dq * gm.gpf;
  uint32_t gf = wave0 / gm.gpf, gr = wave0 - gf * gm.gpf;
  for (uint32_t g0 = wave0; g0 < n_groups; g0 += n_waves) {
    const uint32_t grp = g0;
    const uint32_t f = gf;
    const int r0 = (int)gr * kGroupRows;
    const int64_t row0 = (int64_t)f * gm.rows + r0;
    const int nr = min(kGroupRows, gm.rows - r0);
    gf += dq;
    gr += dr;
    if (gr >= gm.gpf) {
      gr -= gm.gpf;
      ++gf;
    }
    uint4 v[kGroupRows];
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k) {
      // streamed once: non-temporal loads keep the echo out of L2's reuse set
      const u32x4 q = (k < nr) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(
                                     echo + (row0 + k) * 1024 + lane * 16))
                               : u32x4{0u, 0u, 0u, 0u};
      v[k] = make_uint4(q.x, q.y, q.z, q.w);
    }
    if constexpr (STAGE) {
      uint32_t m[kGroupRows];
      int incl[kGroupRows];
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k)
        m[k] = (k < nr) ? mask16(keep_bits<HI>(v[k].x, K), keep_bits<HI>(v[k].y, K),
                                 keep_bits<HI>(v[k].z, K), keep_bits<HI>(v[k].w, K))
                        : 0u;  // a zero sample is kept when T = -1: rows past nr keep nothing
      // two rows per scan: a row's inclusive lane count is <= 1024, so the low and high halves
      // of one 32-bit DPP scan never carry into each other (the pass is half VALU-bound: PMC)
      static_assert(kGroupRows == 4, "rows are scanned in pairs");
      uint32_t rb[kGroupRows + 1];
      rb[0] = 0;
#pragma unroll
      for (int k = 0; k < kGroupRows; k += 2) {
        const int pair = wave_incl_scan_dpp(__popc(m[k]) | (__popc(m[k + 1]) << 16));
        incl[k] = pair & 0xffff;
        incl[k + 1] = (int)((uint32_t)pair >> 16);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane(pair, 63);
        rb[k + 1] = rb[k] + (tot & 0xffffu);
        rb[k + 2] = rb[k + 1] + (tot >> 16);
      }
      const uint32_t total = rb[kGroupRows];
      if (total != 0u && total <= (uint32_t)kStageSlots) {  // wave-uniform
        uint32_t* e = entries + (int64_t)grp * kStageSlots;
        __shared__ GroupLds s_lds[kWavesPerBlock];
        GroupLds& L = s_lds[threadIdx.x / 64];
        group_to_lds(L, lane, m, incl, v);
        const StageBases sb(total);
        for (uint32_t i = (uint32_t)lane; i < total; i += 64u)
          e[ph4 ? sb.pos(i) : i] = kept_entry(L, rb, i);
        wave_lds_sync();  // the slice is rewritten by the next group
      }
      if (lane == 0) group_count[grp] = (int32_t)total;
      continue;
    } else {
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k) {
        if (k >= nr) break;  // a zero sample is kept when T = -1
        c += __popc(keep_bits<HI>(v[k].x, K)) + __popc(keep_bits<HI>(v[k].y, K)) +
             __popc(keep_bits<HI>(v[k].z, K)) + __popc(keep_bits<HI>(v[k].w, K));
      }
      int s = (int)c;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) group_count[grp] = s;
    }
  }
}

// Staged count pass, emitted layout: besides the group counts it leaves, per group, only the
// entries the write pass will emit (a quarter of the kept samples at the reference's stride 4:
// a quarter of the rank searches and of the stores, and the write pass reads consecutive
// entries).  Which kept samples those are depends on the group's in-file rank, so a file's
// groups are counted IN ORDER by one workgroup of W waves (gridDim.x = n_files): in round r wave
// w takes group r * W + w of the file, and the rank of the file's kept samples before the round
// is carried by the workgroup.  W > 1: every wave leaves its group total in LDS, one block
// barrier follows and a wave's rank is the round's base plus the totals of the waves below it
// (totals double-buffered by round parity: a wave a round ahead writes the other half, and it
// can be no further ahead than that).  Every wave runs every round's barrier; a wave without a
// group in a short last round contributes 0.  No wave waits for another workgroup.
//
// A group whose outputs [first, first + m) end inside the file's region of C = gpf * kStageSlots
// words (k1_emit.h emit_staged_file) stores exactly those m kept_entry() words, with the group's
// first row added to the row field, at words first .. first + m - 1 of the region: a file's
// stores are one contiguous run in output order.  The groups from the first one that does not
// fit are left to the write pass's echo re-read.
// The next round's rows are loaded before this round's are used (16 VGPRs).
template <int W>
struct CountTotals {
  uint32_t t[2][W];
};
template <bool HI, int W>
__global__ __launch_bounds__(64 * W) void k_group_count_u8_files(
    const uint8_t* __restrict__ echo, GroupMap gm, uint32_t K, EmitStride es,
    int32_t* __restrict__ group_count, uint32_t* __restrict__ entries) {
  __shared__ GroupLds s_lds[W];
  __shared__ CountTotals<W> s_tot;
  const int lane = threadIdx.x & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t f = blockIdx.x;
  const int64_t file_row0 = (int64_t)f * gm.rows;
  const uint32_t n_rounds = (gm.gpf + W - 1) / W;
  const uint32_t fcap = gm.gpf * (uint32_t)kStageSlots;  // words of a file's region
  auto load_group = [&](uint32_t gi, u32x4 (&q)[kGroupRows]) -> int {  // gi: any value
    const int r0 = (int)gi * kGroupRows;
    const int nr = gi < gm.gpf ? min(kGroupRows, gm.rows - r0) : 0;
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k)
      // streamed once: non-temporal loads keep the echo out of L2's reuse set
      q[k] = (k < nr) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(
                            echo + (file_row0 + r0 + k) * 1024 + lane * 16))
                      : u32x4{0u, 0u, 0u, 0u};
    return nr;
  };
  u32x4 nx[kGroupRows];
  int nr_next = load_group(w, nx);
  uint32_t rank = 0u;  // the file's kept samples before this round (W == 1: before this group)
  for (uint32_t r = 0u; r < n_rounds; ++r) {
    const uint32_t gi = r * W + w;
    const int nr = nr_next;  // 0: no group for this wave in this (last) round
    uint4 v[kGroupRows];
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k) v[k] = make_uint4(nx[k].x, nx[k].y, nx[k].z, nx[k].w);
    nr_next = load_group(gi + W, nx);
    uint32_t m[kGroupRows];
    int incl[kGroupRows];
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k)
      m[k] = (k < nr) ? mask16(keep_bits<HI>(v[k].x, K), keep_bits<HI>(v[k].y, K),
                               keep_bits<HI>(v[k].z, K), keep_bits<HI>(v[k].w, K))
                      : 0u;  // a zero sample is kept when T = -1: rows past nr keep nothing
    // two rows per scan: a row's inclusive lane count is <= 1024, so the low and high halves
    // of one 32-bit DPP scan never carry into each other (the pass is half VALU-bound: PMC)
    static_assert(kGroupRows == 4, "rows are scanned in pairs");
    uint32_t rb[kGroupRows + 1];
    rb[0] = 0;
#pragma unroll
    for (int k = 0; k < kGroupRows; k += 2) {
      const int pair = wave_incl_scan_dpp(__popc(m[k]) | (__popc(m[k + 1]) << 16));
      incl[k] = pair & 0xffff;
      incl[k + 1] = (int)((uint32_t)pair >> 16);
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane(pair, 63);
      rb[k + 1] = rb[k] + (tot & 0xffffu);
      rb[k + 2] = rb[k + 1] + (tot >> 16);
    }
    const uint32_t total = rb[kGroupRows];
    uint32_t my_rank = rank;
    if constexpr (W > 1) {
      const uint32_t par = r & 1u;
      if (lane == 0) s_tot.t[par][w] = total;
      __syncthreads();
      uint32_t below = 0u, all = 0u;
      static_assert(W <= 4, "the wave totals are summed as scalars");
#pragma unroll
      for (uint32_t j = 0u; j < (uint32_t)W; ++j) {
        const uint32_t t = __builtin_amdgcn_readfirstlane(s_tot.t[par][j]);
        below += j < w ? t : 0u;
        all += t;
      }
      my_rank += below;
      rank += all;
    } else {
      rank += total;
    }
    if (nr == 0) continue;  // wave-uniform; the barrier above is behind us
    const EmitSpan sp = emit_span(my_rank, total, es);
    const int64_t grp = (int64_t)f * gm.gpf + gi;
    if (emit_staged_file(sp, fcap)) {  // wave-uniform
      uint32_t* e = entries + (int64_t)f * fcap + sp.first;
      const uint32_t row_bits = (gi * kGroupRows) << 18;  // rows <= 2^14 (staged_emitted)
      GroupLds& L = s_lds[w];
      group_to_lds(L, lane, m, incl, v);
      for (uint32_t j = (uint32_t)lane; j < sp.m; j += 64u)
        e[j] = kept_entry(L, rb, sp.rank0 + j * es.stride) | row_bits;
      wave_lds_sync();  // the slice is rewritten by the next group
    }
    if (lane == 0) group_count[grp] = (int32_t)total;
  }
}

// Which layout a staged K1 uses.  The file-ordered pass has whole files (4 MiB at 4096 rows) as
// its work units, ceil(n_files / 256) of them on the busiest of the 256 CUs: it streams the echo
// 8 to 16 % faster than the by-rank pass when the CUs are evenly loaded and loses that, and more,
// when they are not.  Count pass, file-ordered / by rank, us (profiles/r13/k1_file_order/):
//   files   on the busiest CU / average   file-ordered   by rank
//    375            2 / 1.46                   433          324
//   1500            6 / 5.86                  1238         1326
//   1794            8 / 7.01                  1716         1597
//   2052            9 / 8.02                  1859         1900
//   3000           12 / 11.72          2498 .. 2596   2835 .. 2899
//   6000           24 / 23.44                 4853         5510
// So: the emitted layout when the busiest CU has at most 1/19 more than the average, from the
// smallest stack it was measured ahead at, for sweeps of at most 2^14 rows (the entry's row
// field): staged_emitted(n_files, rows) in k1_emit.h, host arithmetic with its own host check.

// Waves per file of the file-ordered count pass: the most of 4, 2, 1 with every workgroup
// resident at once (a CU holds 32 waves and 160 KiB of LDS, a wave's GroupLds is 5 KiB: 7
// workgroups of 4 waves, 15 of 2, 31 of 1).  A second round of workgroups would start when the
// first ends: a tail as long as a whole file (W = 4 at 3000 files: 2512 us for W = 2's 2498;
// W = 1 there, 3000 of the 8192 wave slots: 2933).  More waves per file could only be resident
// in stacks that take the by-rank layout (W = 8 and 16 at 375 files: 433 and 462 us).
//   files on the busiest CU   6, 7 (n_files <= 1792)   8 .. 15 (<= 3840)   16 and more
//   W                                4                       2               1
// (emitted n_files: 1500 .. 1536, 1703 .. 1792 | 1946 .. 2048, 2189 .. 2304, ..., 2919 .. 3072,
// ..., 3648 .. 3840 | 3892 .. 4096, ..., and every n_files from 4865 on)
inline int count_waves_per_file(int64_t n_files) {
  const int64_t per_cu = busiest_cu_files(n_files);
  return per_cu <= 7 ? 4 : (per_cu <= 15 ? 2 : 1);
}

// file_offsets input: per file ceil(kept / stride) from the group prefix
__global__ void k_file_counts_groups(const int64_t* __restrict__ gprefix, int64_t n_files,
                                     uint32_t gpf, int stride, int64_t* __restrict__ file_out) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_files;
       f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kept = gprefix[(f + 1) * gpf] - gprefix[f * gpf];
    file_out[f] = (kept + stride - 1) / stride;
  }
}
