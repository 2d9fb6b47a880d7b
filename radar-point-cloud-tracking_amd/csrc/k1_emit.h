// Which kept samples of a 4-row group K1 emits, which of them the count pass stages and in which
// layout: the pure arithmetic shared by the staged count pass, k_group_starts, k_file_staged and
// k_group_write_u8 (polar_count.inc, polar_expand.inc, polar_write.inc), and by the host check
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

// Words of the staging buffer per group.  In the by-rank layout a group has a slot of that many
// words and is staged when it keeps 1 .. kStageSlots samples (polar_count.inc).  In the
// file-contiguous layout (file-ordered count pass) a FILE has the gpf * kStageSlots words of its
// gpf groups as one region that holds the file's emitted entries in output order, see
// emit_staged_file.
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

// ---- the file-contiguous layout: entry j of a group is word s.first + j of its file's region of
// `cap` words (cap = gpf * kStageSlots), so the region is the file's outputs 0, 1, 2 ... in order.
// The staging rule: the group's outputs end inside the region.  first + m is the file's output
// count through this group, which never decreases along the file: once a group is not staged no
// later emitting group of the file is.  It depends on (rank, total, stride, cap) only, so the
// write pass re-derives it from the group prefix.  (first + m <= 2^32 - 1: no overflow.)
RPT_K1_HD bool emit_staged_file(const EmitSpan& s, uint32_t cap) {
  return s.m != 0u && s.first + s.m <= cap;
}
// the group emits outputs that are not staged (the write pass reads them from the echo)
RPT_K1_HD bool emit_unstaged_file(const EmitSpan& s, uint32_t cap) {
  return s.m != 0u && s.first + s.m > cap;
}
// A file's staged outputs are its outputs [0, staged_out): all `count` of them when no group is
// unstaged (count <= cap), else the first output of the first unstaged group.  As a fold over the
// file's groups in any order, starting from so = count.
RPT_K1_HD uint32_t emit_staged_out(uint32_t so, const EmitSpan& s, uint32_t cap) {
  return (emit_unstaged_file(s, cap) && s.first < so) ? s.first : so;
}

// ---- which layout a staged K1 uses: a pure function of the call's arguments, the same in the
// count and the write call.  The file-ordered count pass has whole files as its work units,
// ceil(n_files / kCus) of them on the busiest CU; it is ahead of the by-rank pass when the busiest
// CU has at most 1/19 more than the average, from the smallest stack it was measured ahead at
// (the table is in polar_count.inc).  The file-contiguous entry holds the row within the FILE in
// 14 bits: taller sweeps take the by-rank layout.
constexpr int64_t kCus = 256;  // MI355X
constexpr int64_t kEmittedMinFiles = 1500;
constexpr int kEntryRowBits = 14;
constexpr int kEmittedMaxRows = 1 << kEntryRowBits;
inline int64_t busiest_cu_files(int64_t n_files) { return (n_files + kCus - 1) / kCus; }
inline bool staged_emitted(int64_t n_files, int64_t rows) {
  return n_files >= kEmittedMinFiles && n_files * 20 >= busiest_cu_files(n_files) * kCus * 19 &&
         rows <= kEmittedMaxRows;
}

}  // namespace rpt
