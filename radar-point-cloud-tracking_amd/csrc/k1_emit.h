// Which kept samples of a 4-row group K1 emits: the pure arithmetic shared by the staged count
// pass, k_group_starts and k_group_write_u8 (polar.hip), and by the host check
// tools/asan/k1_emit_main.cpp, so everything here is plain C++.
//
// A file's kept samples are numbered in file order (the in-file rank); K1 emits those whose rank
// is a multiple of stride, and output o of the file is the kept sample of rank o * stride.  A group
// whose first kept sample has in-file rank `rank` and which keeps `total` samples therefore owns
// the file's outputs [first, last), first = ceil(rank / stride), last = ceil((rank + total) /
// stride); its j-th output is the kept sample of IN-GROUP rank rank0 + j * stride, rank0 =
// first * stride - rank < stride.  rank + total is below 2^32 (a file has fewer samples than
// that); nothing here adds stride to a rank, so no stride overflows the 32-bit arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_K1_HD __host__ __device__ __forceinline__
#else
#define RPT_K1_HD inline
#endif

namespace rpt {

// Entries per group slot of the staging buffer.  In the emitted layout (file-ordered count pass)
// a group is staged when it emits 1 .. kStageSlots outputs and its slot holds exactly those, see
// emit_staged; in the by-rank layout when it keeps 1 .. kStageSlots samples (polar.hip).
constexpr int kStageSlots = 512;

// stride >= 1; power-of-two strides (the reference's POINT_STRIDE = 4) divide by shifts
struct EmitStride {
  uint32_t stride;
  uint32_t shift;  // log2(stride) when pow2
  bool pow2;
};
RPT_K1_HD EmitStride emit_stride(uint32_t stride) {
  return EmitStride{stride, (uint32_t)__builtin_ctz(stride), (stride & (stride - 1u)) == 0u};
}

struct EmitSpan {
  uint32_t first;  // the group's first output, as an in-file output index
  uint32_t m;      // outputs of the group: last - first
  uint32_t rank0;  // in-group kept rank of the first output (meaningful when m != 0)
};

// ceil(a / stride) and, through *rem, a mod stride
RPT_K1_HD uint32_t emit_ceil(uint32_t a, const EmitStride& es, uint32_t* rem) {
  const uint32_t q = es.pow2 ? (a >> es.shift) : a / es.stride;
  const uint32_t r = es.pow2 ? (a & (es.stride - 1u)) : a - q * es.stride;
  if (rem) *rem = r;
  return q + (r != 0u ? 1u : 0u);
}

RPT_K1_HD EmitSpan emit_span(uint32_t rank, uint32_t total, const EmitStride& es) {
  uint32_t rem;
  EmitSpan s;
  s.first = emit_ceil(rank, es, &rem);
  s.m = emit_ceil(rank + total, es, nullptr) - s.first;
  s.rank0 = rem != 0u ? es.stride - rem : 0u;
  return s;
}

// The one staging rule: the group's slot holds its m emitted entries at positions 0 .. m-1.
// It depends on the rank's residue, not on the kept count alone: 2049 kept samples at stride 4
// are 513 outputs after a rank that is a multiple of 4 and 512 otherwise.
RPT_K1_HD bool emit_staged(const EmitSpan& s) { return s.m != 0u && s.m <= (uint32_t)kStageSlots; }

}  // namespace rpt
