// K1, what more than one stage file or the driver (polar.hip count_impl / write_impl) reads.
// One kernel, k_bounds_parts (launched by write_impl after the expand and list writes): it reads
// the per-block xy-bounds partials that the write kernels leave through XyBounds::store_block and
// leaves the stack's bounds {min x, max x, min y, max y} as ordered u32 in out[0..3].
//   block size, sample conversion, per-lane vector loads   kBlock, kWavesPerBlock, to_f, Vec<T>
//   wave prefix sums                                        wave_excl_scan (generic rows),
//                                                           wave_incl_scan_dpp (grouped u8)
//   u8 keep test and mask helpers                           keep_bits, mask16, nth_bit16
//   groups of kGroupRows rows of one file                   kGroupRows, GroupMap, group_rows
//   a wave's group in LDS, kept sample by in-group rank     GroupLds, wave_lds_sync, group_to_lds,
//                                                           kept_entry (the entry word's format)
//   xy bounds folded into the write kernels                 f2ord, XyBounds, k_bounds_parts
//   the two staging layouts (the note before phase_base)    phase_base, stage_pos, StageBases
// Read by two stages or more: kBlock, wave_incl_scan_dpp and keep_bits .. kept_entry (count,
// write), GroupMap (count, write, expand), XyBounds (write, expand), the staging positions (count
// through StageBases, write through stage_pos, expand through phase_base).  Vec is read by the row
// kernels and by the driver's alignment rule; to_f and wave_excl_scan by the row kernels alone.
// Reads common.h (kWave) and k1_emit.h (kStageSlots); no stage file.

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

template <class T>
__device__ __forceinline__ float to_f(T v) {
  return (float)v;
}

// Elements per lane per iteration: 16 u8 (one uint4) or 4 f32 (one float4).
template <class T>
struct Vec;
template <>
struct Vec<uint8_t> {
  static constexpr int N = 16;
  using L = uint4;
  __device__ static void unpack(const L& v, float (&o)[16]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
  }
};
template <>
struct Vec<float> {
  static constexpr int N = 4;
  using L = float4;
  __device__ static void unpack(const L& v, float (&o)[4]) {
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
    o[3] = v.w;
  }
};

__device__ __forceinline__ int wave_excl_scan(int v, int* total) {
  const int lane = threadIdx.x & 63;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}

// Inclusive wave prefix sum with DPP (6 VALU ops, no LDS): row_shr 1/2/4/8 within 16-lane rows,
// then row_bcast:15 / row_bcast:31 carry the row totals (GFX9-family DPP, available on gfx950).
__device__ __forceinline__ int wave_incl_scan_dpp(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return v;
}

// ---- u8 fast path (the radar's native sample type), bins == 1024: one 16-B load per lane per
// row.  For integer samples v in [0, 255], (float)v > thr  <=>  v > T with T = floor(thr) clamped
// to [-1, 255] (NaN -> 255: nothing kept), evaluated on 4 bytes at once (SWAR, exact per byte,
// no carries across bytes), K = (HI ? 255 - T : 127 - T) * 0x01010101:
//   T <= 127 : hi bit of ((x & 0x7f..) + K) | x
//   T >= 128 : hi bit of ((x & 0x7f..) + K) & x
template <bool HI>
__device__ __forceinline__ uint32_t keep_bits(uint32_t x, uint32_t K) {
  const uint32_t lo = x & 0x7f7f7f7fu;
  return (HI ? ((lo + K) & x) : ((lo + K) | x)) & 0x80808080u;
}
// The 16 per-byte keep bits of a lane (bytes 0x80 or 0 in m0..m3) -> a 16-bit mask, sample k ->
// bit k: two dot4 products per 8 samples (weights 1..8 and 16..128 on the 0x80 bytes) instead of
// a multiply-gather per dword.
__device__ __forceinline__ uint32_t mask16(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3) {
  const uint32_t lo = __builtin_amdgcn_udot4(
      m0, 0x08040201u, __builtin_amdgcn_udot4(m1, 0x80402010u, 0u, false), false);
  const uint32_t hi = __builtin_amdgcn_udot4(
      m2, 0x08040201u, __builtin_amdgcn_udot4(m3, 0x80402010u, 0u, false), false);
  return (lo | (hi << 8)) >> 7;
}

// Position of the n-th (0-based) set bit of a 16-bit mask, n < popcount: binary search on
// popcounts of the low half, quarter, ... (v_cndmask selects, no branches).
__device__ __forceinline__ int nth_bit16(uint32_t m, uint32_t n) {
  int p = 0;
  uint32_t c = __popc(m & 0xffu);
  if (n >= c) { n -= c; p = 8; }
  c = __popc((m >> p) & 0xfu);
  if (n >= c) { n -= c; p += 4; }
  c = __popc((m >> p) & 0x3u);
  if (n >= c) { n -= c; p += 2; }
  c = (m >> p) & 1u;
  if (n >= c) p += 1;
  return p;
}

// Rows are handled in groups of kGroupRows consecutive rows of one file (the last group of a file
// may be short): a wave issues the group's loads together (4 KiB in flight) before ranking any of
// them.  The count pass writes one kept count per GROUP; the write pass walks the group's rows in
// order and carries the in-file rank across them, so no per-row reduction or prefix is needed.
constexpr int kGroupRows = 4;  // k_group_write_u8 selects the rows' geometry among 4
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct GroupMap {
  uint32_t gpf;   // groups per file = ceil(rows / kGroupRows)
  int rows;
};
// file, first row of the group in the stack and its row count (all wave-uniform)
__device__ __forceinline__ void group_rows(const GroupMap& gm, uint32_t grp, uint32_t* f,
                                           int64_t* row0, int* nr) {
  const uint32_t ff = grp / gm.gpf;
  const int r0 = (int)(grp - ff * gm.gpf) * kGroupRows;
  *f = ff;
  *row0 = (int64_t)ff * gm.rows + r0;
  *nr = min(kGroupRows, gm.rows - r0);
}

// Kept samples of a group by in-group rank.  A wave leaves its group's per-row inclusive lane
// counts, keep masks and sample bytes in its LDS slice; the kept sample of in-group rank i is then
// found by any lane: row from the row bases (scalar compares), lane by a 6-step binary search of
// the row's inclusive counts, bit by nth_bit16 of that lane's mask.  Work goes to the OUTPUT slots
// (consecutive lanes, full-width stores) instead of walking each input lane's mask bits, so a
// dense lane no longer holds its whole wave in a divergent loop.
struct GroupLds {  // 5 KiB per wave: 8 waves per SIMD fit the LDS (u16 counts and masks)
  uint16_t incl[kGroupRows][64];  // <= 1024
  uint16_t mask[kGroupRows][64];
  uint32_t bytes[kGroupRows][256];  // the group's 4 KiB of samples
};

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// xy bounds of the written points, folded into the K1 write kernels (the land grid's edges need
// them; a separate pass re-read x and y: ~0.1 ms at 1000 frames).  Floats as order-preserving
// u32 (-0 below +0), as k_bounds_xy: {min x, max x, min y, max y}; each block leaves one
// partial, k_bounds_parts reduces them.
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
struct XyBounds {
  uint32_t v[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};
  __device__ void add(float x, float y) {
    const uint32_t a = f2ord(x), b = f2ord(y);
    v[0] = min(v[0], a);
    v[1] = max(v[1], a);
    v[2] = min(v[2], b);
    v[3] = max(v[3], b);
  }
  // whole block (every thread calls it once, after its last add): partial of block blockIdx.x.
  // scratch: 4 LDS words per wave at scratch + 4 * wstride * wave, free for the caller by now
  // (a kernel's own LDS, so the reduction does not add to its LDS size and cost occupancy)
  __device__ void store_block(uint32_t* __restrict__ part, uint32_t* scratch, int wstride) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v[0] = min(v[0], (uint32_t)__shfl_xor((int)v[0], off));
      v[1] = max(v[1], (uint32_t)__shfl_xor((int)v[1], off));
      v[2] = min(v[2], (uint32_t)__shfl_xor((int)v[2], off));
      v[3] = max(v[3], (uint32_t)__shfl_xor((int)v[3], off));
    }
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < 4; ++k) scratch[4 * wstride * (threadIdx.x / 64) + k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
      const int k = threadIdx.x;
      uint32_t r = scratch[k];
      for (int w = 1; w < kWavesPerBlock; ++w) {
        const uint32_t o = scratch[4 * wstride * w + k];
        r = (k & 1) ? max(r, o) : min(r, o);
      }
      part[4 * blockIdx.x + k] = r;
    }
  }
};
__global__ __launch_bounds__(kBlock) void k_bounds_parts(const uint32_t* __restrict__ part, int nb,
                                                        uint32_t* __restrict__ out) {
  XyBounds b;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    b.v[0] = min(b.v[0], part[4 * i + 0]);
    b.v[1] = max(b.v[1], part[4 * i + 1]);
    b.v[2] = min(b.v[2], part[4 * i + 2]);
    b.v[3] = max(b.v[3], part[4 * i + 3]);
  }
  __shared__ uint32_t sm[4 * kWavesPerBlock];
  b.store_block(out - 4 * blockIdx.x, sm, 1);  // one block: out[0..3]
}

__device__ __forceinline__ void group_to_lds(GroupLds& L, int lane, const uint32_t (&m)[kGroupRows],
                                             const int (&incl)[kGroupRows],
                                             const uint4 (&vv)[kGroupRows]) {
#pragma unroll
  for (int k = 0; k < kGroupRows; ++k) {
    L.incl[k][lane] = (uint16_t)incl[k];
    L.mask[k][lane] = (uint16_t)m[k];
    *reinterpret_cast<uint4*>(&L.bytes[k][lane * 4]) = vv[k];
  }
  wave_lds_sync();
}

// (row << 18) | (bin << 8) | sample of the kept sample of in-group rank i (i < rb[kGroupRows];
// rb[k] = kept samples of the rows before row k)
__device__ __forceinline__ uint32_t kept_entry(const GroupLds& L,
                                               const uint32_t (&rb)[kGroupRows + 1], uint32_t i) {
  const int k = (i >= rb[1]) + (i >= rb[2]) + (i >= rb[3]);
  const int ir = (int)(i - rb[k]);
  const uint16_t* inc = L.incl[k];
  int lo = 0;  // lanes whose inclusive count is <= ir
#pragma unroll
  for (int step = 32; step > 0; step >>= 1)
    if (inc[lo + step - 1] <= ir) lo += step;
  const uint32_t msk = L.mask[k][lo];
  const int j = ir - ((int)inc[lo] - __popc(msk));
  const int bit = nth_bit16(msk, (uint32_t)j);
  const int bin = lo * 16 + bit;
  const uint32_t w = L.bytes[k][bin >> 2];
  return ((uint32_t)k << 18) | ((uint32_t)bin << 8) | __builtin_amdgcn_ubfe(w, 8u * (bin & 3), 8u);
}

// Staged kept samples (nullable): the count pass also stores kept samples as kept_entry() words
// in a buffer of kStageSlots words per group (k1_emit.h); the write pass then reads those instead
// of the group's 4 KiB of echo (one read of the echo for the whole K1).  A group that is not
// staged (dense sweeps) is read from the echo again by the write pass.  Two layouts, chosen from
// n_files and rows alone (k1_emit.h staged_emitted()), the same in the count and the write call:
//   by rank  (k_group_count_u8<HI, true>, groups to waves in any order): a group has a slot of
//            kStageSlots words; one that keeps at most kStageSlots samples stores ALL of them in
//            in-group rank order, and the write pass (k_group_starts + k_expand_write) reads the
//            emitted ones, every stride-th.
//   emitted, file-contiguous  (k_group_count_u8_files, a file's groups counted in order): file f
//            has the C = gpf * kStageSlots words from f * C on.  A group that emits the file's
//            outputs [first, first + m), m != 0 and first + m <= C (emit_staged_file), stores
//            exactly those m entries at words first .. first + m - 1: the region is the file's
//            outputs in order, word o = output o, global slot file_offsets[f] + o.  The entry's
//            row field is the row within the FILE (14 bits; its low two bits are still the row
//            within the group).  Nothing else is written to the buffer.  The write pass
//            (k_file_staged + k_expand_stream) streams the regions: no per-group search.
// Slot position (by rank) of in-group kept rank i in a staged group of `total` entries.  With stride 4 (the
// reference's POINT_STRIDE) the ranks of each residue mod 4 are contiguous and the four residues
// packed back to back in [0, total): the write pass reads every 4th rank from one residue, i.e.
// consecutive entries, instead of one entry in four from every line of the slot, while the count
// pass still fills one contiguous region per group (a fixed 64-entry stride per residue left four
// partly written lines per sparse group: +9 % on the count pass).
__device__ __forceinline__ uint32_t phase_base(uint32_t ph, uint32_t total) {
  uint32_t b = 0u;
#pragma unroll
  for (uint32_t j = 0u; j < 3u; ++j) b += (j < ph) ? ((total + 3u - j) >> 2) : 0u;
  return b;
}
__device__ __forceinline__ uint32_t stage_pos(uint32_t i, uint32_t total, bool ph4) {
  return ph4 ? phase_base(i & 3u, total) + (i >> 2) : i;
}
// the same with the group's residue bases computed once (wave-uniform: scalar registers)
struct StageBases {
  uint32_t b1, b2, b3;
  __device__ explicit StageBases(uint32_t total)
      : b1((total + 3u) >> 2), b2(b1 + ((total + 2u) >> 2)), b3(b2 + ((total + 1u) >> 2)) {}
  __device__ uint32_t pos(uint32_t i) const {
    const uint32_t r = i & 3u;
    return (r == 0u ? 0u : (r == 1u ? b1 : (r == 2u ? b2 : b3))) + (i >> 2);
  }
};
