// K1 write pass on grouped u8 sweeps, one wave per group: k_group_write_u8, launched by
// write_impl of polar.hip in three roles:
//   <HI, false, false>  no entries buffer: every group is ranked again from the echo
//   <HI, true,  false>  entries given, the expand write off or out of its bounds: staged groups
//                       are read from the entries (either layout), the others from the echo
//   <HI, false, true>   LIST, after an expand write (polar_expand.inc): only the unstaged groups
//                       that k_group_starts / k_file_staged listed, from the echo
// Reads the group prefix (row_prefix), file_offsets, the rows' scale / cos / sin and the files'
// gains.  Writes x, y, val (float or the u8 sample), gain and point frame of the emitted samples
// below cap, and, when bpart is given, one xy-bounds partial per block for k_bounds_parts.
// Reads polar_shared.inc and k1_emit.h (emit_stride, emit_span, emit_staged_file).

// Write pass: the kept samples whose in-file rank is a multiple of stride.  The group's emitted
// outputs [first, last) (in-file indices: ceil(rank / stride) ...) go to consecutive lanes; output
// o is the kept sample of in-group rank o * stride - rank, found with kept_entry() from the
// group's LDS slice (or, STAGED, read from the count pass's slot when the group was staged:
// no echo read at all).  Outputs at or beyond cap are dropped: a speculative launch (sized by an
// earlier run) is repeated by the caller when the count says it did not fit.
// LIST: the groups are the first *list_n entries of list (the unstaged groups of the expand
// write below), not 0 .. n_groups-1.
// VT: the element type of val, float or -- the stack driver's narrow path -- uint8_t (the
// sample itself, the entry's low byte).
template <bool HI, bool STAGED, bool LIST = false, class VT = float>
__global__ __launch_bounds__(kBlock, 8) void k_group_write_u8(
    const uint8_t* __restrict__ echo, uint32_t n_groups, GroupMap gm, uint32_t K, int stride,
    const float* __restrict__ scale, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, const int32_t* __restrict__ gain,
    const int64_t* __restrict__ gprefix, const int64_t* __restrict__ file_offsets,
    int files_per_frame, float* __restrict__ x, float* __restrict__ y, VT* __restrict__ val,
    int32_t* __restrict__ gain_out, int32_t* __restrict__ pf_out, int64_t cap,
    const uint32_t* __restrict__ entries, bool emitted,
    const uint32_t* __restrict__ list = nullptr, const uint32_t* __restrict__ list_n = nullptr,
    uint32_t* __restrict__ bpart = nullptr) {
  // emitted (kernel-uniform; STAGED only): the entries' layout, see "Staged kept samples"
  // bpart (nullable, kernel-uniform): this block's xy-bounds partial (XyBounds)
  __shared__ GroupLds s_lds[kWavesPerBlock];
  XyBounds xb;
  const int lane = threadIdx.x & 63;
  GroupLds& L = s_lds[threadIdx.x / 64];
  const uint32_t wave0 = blockIdx.x * kWavesPerBlock + threadIdx.x / 64;
  const uint32_t n_waves = gridDim.x * kWavesPerBlock;
  const uint32_t us = (uint32_t)stride;
  const EmitStride es = emit_stride(us);
  const float inv_bins = 1.0f / 1024.0f;  // exact: step = scale / 1024 == scale * 2^-10
  const uint32_t n_items = LIST ? *list_n : n_groups;
  for (uint32_t g0 = wave0; g0 < n_items; g0 += n_waves) {
    const uint32_t grp = __builtin_amdgcn_readfirstlane(LIST ? list[g0] : g0);
    uint32_t f;
    int64_t row0;
    int nr;
    group_rows(gm, grp, &f, &row0, &nr);
    // the group's rows' geometry, loaded by lanes 0..3 together with the prefix reads (one
    // dependent load level less per output: ent -> row -> geometry becomes a lane shuffle)
    float g_sc = 0.f, g_c = 0.f, g_s = 0.f;
    if (lane < nr) {
      g_sc = scale[row0 + lane];
      g_c = cos_t[row0 + lane];
      g_s = sin_t[row0 + lane];
    }
    float r_sc[kGroupRows], r_c[kGroupRows], r_s[kGroupRows];  // wave-uniform (readlane)
#pragma unroll
    for (int k = 0; k < kGroupRows; ++k) {
      r_sc[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g_sc), k));
      r_c[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g_c), k));
      r_s[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g_s), k));
    }
    // in-file rank of the group's first kept sample (< rows * 1024 < 2^32), its kept count, the
    // group's emitted outputs [first, last) and the file's output base
    const int64_t gp0 = gprefix[grp];
    const uint32_t rank = (uint32_t)(gp0 - gprefix[(int64_t)f * gm.gpf]);
    const uint32_t total = (uint32_t)(gprefix[grp + 1] - gp0);
    const EmitSpan sp = emit_span(rank, total, es);
    if (sp.m == 0u) continue;  // wave-uniform: nothing emitted
    const uint32_t first = sp.first, last = sp.first + sp.m;
    const int64_t out0 = file_offsets[f];
    const int32_t g = gain ? gain[f] : 0;
    const int32_t fr = (int32_t)(f / (uint32_t)files_per_frame);
    const uint32_t fcap = gm.gpf * (uint32_t)kStageSlots;  // (emitted) words of a file's region
    const bool staged = STAGED && (emitted ? emit_staged_file(sp, fcap)
                                           : total <= (uint32_t)kStageSlots);  // wave-uniform
    uint32_t rb[kGroupRows + 1];
    if (!staged) {
      uint4 vv[kGroupRows];
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k)
        vv[k] = (k < nr) ? *reinterpret_cast<const uint4*>(echo + (row0 + k) * 1024 + lane * 16)
                         : make_uint4(0u, 0u, 0u, 0u);
      uint32_t m[kGroupRows];
      int incl[kGroupRows];
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k) {
        m[k] = (k < nr) ? mask16(keep_bits<HI>(vv[k].x, K), keep_bits<HI>(vv[k].y, K),
                                 keep_bits<HI>(vv[k].z, K), keep_bits<HI>(vv[k].w, K))
                        : 0u;
        incl[k] = wave_incl_scan_dpp(__popc(m[k]));
      }
      rb[0] = 0;
#pragma unroll
      for (int k = 0; k < kGroupRows; ++k)
        rb[k + 1] = rb[k] + (uint32_t)__builtin_amdgcn_readlane(incl[k], 63);
      group_to_lds(L, lane, m, incl, vv);
    }
    // the group's entries: its slot by rank; emitted, word `first` of its file's region
    const uint32_t* e = entries + ((STAGED && emitted) ? (int64_t)f * fcap + first
                                                       : (int64_t)grp * kStageSlots);
    for (uint32_t o = first + (uint32_t)lane; o < last; o += 64u) {
      const int64_t oo = out0 + o;
      if (oo >= cap) break;
      const uint32_t i = sp.rank0 + (o - first) * us;  // in-group kept rank
      const uint32_t ent = !staged  ? kept_entry(L, rb, i)
                           : emitted ? e[o - first]
                                     : e[stage_pos(i, total, us == 4u)];
      const int rk = (int)((ent >> 18) & 3u);  // (emitted: the row within the file, mod 4)
      const float sc = rk == 0 ? r_sc[0] : (rk == 1 ? r_sc[1] : (rk == 2 ? r_sc[2] : r_sc[3]));
      const float cc = rk == 0 ? r_c[0] : (rk == 1 ? r_c[1] : (rk == 2 ? r_c[2] : r_c[3]));
      const float ss = rk == 0 ? r_s[0] : (rk == 1 ? r_s[1] : (rk == 2 ? r_s[2] : r_s[3]));
      const float rr = sc * inv_bins * (float)((ent >> 8) & 1023u);
      const float px = rr * cc, py = rr * ss;
      x[oo] = px;
      y[oo] = py;
      if (bpart) xb.add(px, py);
      val[oo] = (VT)(ent & 0xffu);
      if (gain_out) gain_out[oo] = g;
      if (pf_out) pf_out[oo] = fr;
    }
    if (!staged) wave_lds_sync();  // the slice is rewritten by the next group
  }
  // (every wave is past its last group: each one's own LDS slice is free)
  if (bpart)
    xb.store_block(bpart, reinterpret_cast<uint32_t*>(&s_lds[0]),
                   (int)(sizeof(GroupLds) / sizeof(uint32_t) / 4));
}
