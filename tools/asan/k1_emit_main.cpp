// Stand-alone AddressSanitizer + UBSan program over K1's emission arithmetic (csrc/k1_emit.h,
// plain C++ shared with the count pass, k_group_starts and k_group_write_u8): a file's kept
// samples are cut into groups at random and every group's span (first output, output count,
// in-group rank of the first output) is checked against a brute-force walk of the file's ranks,
// for power-of-two and other strides, strides above the file's kept count, and the staging edge
// at kStageSlots under every rank residue.
//   make -C tools/asan k1_emit
// `k1_emit_main table` prints "rank total stride first m rank0 staged" for every rank < 40,
// total < 40, stride 1..9 and 64 (tests/test_k1_emit_host.py compares it with numpy).
// `k1_emit_main file` runs the checks of the file-contiguous layout alone (the default run
// includes them): the staging rule and staged_out against a brute-force walk over a file's groups
// around the region's capacity, and the layout predicate (n_files, rows) on both sides of every
// term; it prints the predicate's values (tests/test_k1_file_contiguous_host.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "k1_emit.h"

namespace {

int g_fail = 0;

#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      ++g_fail;                          \
    }                                    \
  } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

// groups[g] = kept samples of group g of one file, in file order
void run_file(const char* name, const std::vector<uint32_t>& groups, uint32_t stride) {
  const rpt::EmitStride es = rpt::emit_stride(stride);
  uint64_t kept = 0;
  for (uint32_t t : groups) kept += t;
  // out_of[i]: the output index of kept sample i of the file, or -1 (exactly `kept` values: a
  // read past the end is caught)
  std::vector<int64_t> out_of((size_t)kept, -1);
  int64_t n_out = 0;
  for (uint64_t i = 0; i < kept; i += stride) out_of[(size_t)i] = n_out++;
  uint32_t rank = 0;
  int64_t next = 0;  // the next output a group may own
  for (size_t g = 0; g < groups.size(); ++g) {
    const uint32_t total = groups[g];
    const rpt::EmitSpan sp = rpt::emit_span(rank, total, es);
    uint32_t m = 0;
    for (uint32_t i = 0; i < total; ++i) m += out_of[(size_t)rank + i] >= 0 ? 1u : 0u;
    CHECK(sp.m == m, "%s: stride %u group %zu: m = %u, expected %u", name, stride, g, sp.m, m);
    CHECK(rpt::emit_staged(sp) == (m != 0u && m <= (uint32_t)rpt::kStageSlots),
          "%s: stride %u group %zu: staged", name, stride, g);
    if (m != 0u && sp.m == m) {
      CHECK((int64_t)sp.first == next, "%s: stride %u group %zu: first = %u, expected %lld", name,
            stride, g, sp.first, (long long)next);
      CHECK(sp.rank0 < stride && sp.rank0 < total, "%s: stride %u group %zu: rank0 = %u", name,
            stride, g, sp.rank0);
      for (uint32_t j = 0; j < m; ++j) {
        const uint64_t i = (uint64_t)sp.rank0 + (uint64_t)j * stride;  // in-group rank
        CHECK(i < total && out_of[(size_t)(rank + i)] == next + j,
              "%s: stride %u group %zu: output %u is not in-group rank %llu", name, stride, g, j,
              (unsigned long long)i);
      }
    }
    next += m;
    rank += total;
  }
  CHECK(next == n_out, "%s: stride %u: %lld outputs, expected %lld", name, stride,
        (long long)next, (long long)n_out);
}

int table() {
  const uint32_t strides[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 64};
  for (uint32_t stride : strides) {
    const rpt::EmitStride es = rpt::emit_stride(stride);
    for (uint32_t rank = 0; rank < 40; ++rank)
      for (uint32_t total = 0; total < 40; ++total) {
        const rpt::EmitSpan sp = rpt::emit_span(rank, total, es);
        std::printf("%u %u %u %u %u %u %d\n", rank, total, stride, sp.first, sp.m,
                    sp.m ? sp.rank0 : 0u, rpt::emit_staged(sp) ? 1 : 0);
      }
  }
  return 0;
}

// The file-contiguous layout: one file's groups against a region of `cap` words.  A brute-force
// walk over the file's outputs says which group owns each one; a group is staged iff it owns
// outputs and the last of them is below cap.  Checked: emit_staged_file / emit_unstaged_file per
// group, that the rule is monotone along the file, the emit_staged_out fold (in file order and
// reversed), and that the staged groups' words first .. first + m - 1 are exactly the region's
// words 0 .. staged_out - 1, word o holding output o.
void run_file_region(const char* name, const std::vector<uint32_t>& groups, uint32_t stride,
                     uint32_t cap) {
  const rpt::EmitStride es = rpt::emit_stride(stride);
  uint64_t kept = 0;
  for (uint32_t t : groups) kept += t;
  const uint64_t n_out = (kept + stride - 1) / stride;
  // the outputs [los[g], his[g]] that group g owns (-1: none), by walking the file's kept ranks
  std::vector<int64_t> los(groups.size(), -1), his(groups.size(), -1);
  {
    uint64_t rank = 0, seen = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
      for (uint64_t i = rank; i < rank + groups[g]; ++i)
        if (i % stride == 0) {
          const int64_t o = (int64_t)(i / stride);
          CHECK(o == (int64_t)seen, "%s: walk", name);  // outputs come in order
          ++seen;
          if (los[g] < 0) los[g] = o;
          his[g] = o;
        }
      rank += groups[g];
    }
    CHECK(seen == n_out, "%s: walk found %llu outputs", name, (unsigned long long)seen);
  }
  std::vector<int64_t> word(cap, -1);  // the region: which output each written word holds
  uint32_t rank = 0, so_fwd = (uint32_t)n_out;
  bool past = false;  // an emitting group before this one was not staged
  int64_t first_unstaged = -1;
  std::vector<rpt::EmitSpan> spans;
  for (size_t g = 0; g < groups.size(); ++g) {
    const rpt::EmitSpan sp = rpt::emit_span(rank, groups[g], es);
    spans.push_back(sp);
    const int64_t lo = los[g], hi = his[g];
    const bool emits = lo >= 0;
    const bool staged = emits && (uint64_t)hi < cap;
    CHECK(rpt::emit_staged_file(sp, cap) == staged, "%s: stride %u cap %u group %zu: staged", name,
          stride, cap, g);
    CHECK(rpt::emit_unstaged_file(sp, cap) == (emits && !staged),
          "%s: stride %u cap %u group %zu: unstaged", name, stride, cap, g);
    if (emits) {
      CHECK(!(past && staged), "%s: stride %u cap %u group %zu: staged after an unstaged group",
            name, stride, cap, g);
      if (!staged && first_unstaged < 0) first_unstaged = lo;
      past = past || !staged;
    }
    if (staged && (int64_t)sp.first == lo && (int64_t)sp.m == hi - lo + 1)
      for (uint32_t j = 0; j < sp.m; ++j) {
        CHECK(word[sp.first + j] < 0, "%s: stride %u cap %u group %zu: word %u written twice",
              name, stride, cap, g, sp.first + j);
        word[sp.first + j] = lo + j;  // (sp.first + j < cap: a write past the end is caught)
      }
    so_fwd = rpt::emit_staged_out(so_fwd, sp, cap);
    rank += groups[g];
  }
  const uint32_t expect = n_out <= cap ? (uint32_t)n_out : (uint32_t)first_unstaged;
  CHECK(so_fwd == expect, "%s: stride %u cap %u: staged_out = %u, expected %u", name, stride, cap,
        so_fwd, expect);
  uint32_t so_rev = (uint32_t)n_out;
  for (size_t g = groups.size(); g-- > 0;) so_rev = rpt::emit_staged_out(so_rev, spans[g], cap);
  CHECK(so_rev == expect, "%s: stride %u cap %u: staged_out folded in reverse = %u, expected %u",
        name, stride, cap, so_rev, expect);
  CHECK(expect <= cap, "%s: stride %u cap %u: staged_out %u beyond the region", name, stride, cap,
        expect);
  for (uint32_t o = 0; o < cap; ++o)
    CHECK(word[o] == (o < expect ? (int64_t)o : -1), "%s: stride %u cap %u: word %u holds %lld",
          name, stride, cap, o, (long long)word[o]);
}

// `k1_emit_main file`: the file-contiguous staging rule around the capacity edge, strides 1..9
// and 64, and both sides of every term of the layout predicate; prints "layout n_files rows e"
// lines (tests/test_k1_file_contiguous_host.py compares them with its own statement of the rule)
int file_checks(bool print) {
  const uint32_t strides[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 64};
  const uint32_t C = 3u * (uint32_t)rpt::kStageSlots;  // 12 rows: 3 groups
  for (uint32_t stride : strides) {
    for (uint32_t cap : {C, (uint32_t)rpt::kStageSlots, 1u}) {
      run_file_region("empty file", {0, 0, 0}, stride, cap);
      run_file_region("one sample", {0, 1, 0}, stride, cap);
      // kept totals on either side of cap outputs, after every residue of the rank before
      for (uint32_t before = 0; before <= stride && before < 12; ++before)
        for (int d = -2; d <= 2; ++d) {
          const int64_t k = (int64_t)cap * stride + d - (int64_t)before;
          if (k < 0 || k > 8192) continue;
          const uint32_t kk = (uint32_t)k, h = kk / 2u;
          run_file_region("edge 2 groups", {before, kk, 5}, stride, cap);
          run_file_region("edge split", {before, h, kk - h, 0, 5 * stride}, stride, cap);
          run_file_region("edge last", {before, kk}, stride, cap);
        }
    }
    // the cases of the device test at stride 1 scaled by the stride
    run_file_region("fits exactly", {1000 * stride, 536 * stride, 0}, stride, C);
    run_file_region("third at C", {1000 * stride, 536 * stride, 5 * stride}, stride, C);
    run_file_region("second straddles", {1000 * stride, 600 * stride, 5 * stride}, stride, C);
    if (1537u * stride <= 4096u) {
      run_file_region("first too long", {1537 * stride, 0, 0}, stride, C);
      run_file_region("first fills", {1536 * stride, 0, 1}, stride, C);
    }
    for (int rep = 0; rep < 200; ++rep) {
      std::vector<uint32_t> g;
      const int n = 1 + (int)(rnd() % 12u);
      for (int k = 0; k < n; ++k) g.push_back(rnd() % 3u == 0u ? 0u : rnd() % 1500u);
      run_file_region("random", g, stride, 1u + rnd() % (2u * C));
    }
  }
  // the layout predicate: n_files (the table of tests/test_k1_file_order_gpu.py) and rows
  struct { int64_t nf; bool e; } const nfs[] = {
      {0, false},    {1499, false}, {1500, true},  {1536, true},  {1537, false}, {1702, false},
      {1703, true},  {1792, true},  {1793, false}, {1945, false}, {1946, true},  {3000, true},
      {3840, true},  {3841, false}, {3891, false}, {3892, true},  {4620, false}, {4621, true},
      {4864, true},  {4865, true},  {100000, true}};
  const int64_t rows[] = {1, 12, 4096, 16383, 16384, 16385, 65536};
  for (const auto& c : nfs)
    for (int64_t r : rows) {
      const bool e = rpt::staged_emitted(c.nf, r);
      CHECK(e == (c.e && r <= 16384), "staged_emitted(%lld, %lld)", (long long)c.nf, (long long)r);
      if (print) std::printf("layout %lld %lld %d\n", (long long)c.nf, (long long)r, e ? 1 : 0);
    }
  // the row field: the last row of the tallest file-contiguous sweep fits above bit 18
  CHECK((((uint64_t)rpt::kEmittedMaxRows - 1u) << 18) <= 0xffffffffull, "row field");
  CHECK(((((uint64_t)rpt::kEmittedMaxRows) << 18) >> 32) != 0u, "row field is not tight");
  return g_fail;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "table") == 0) return table();
  if (argc > 1 && std::strcmp(argv[1], "file") == 0) {
    if (file_checks(true)) {
      std::fprintf(stderr, "k1_emit file: %d check(s) failed\n", g_fail);
      return 1;
    }
    std::puts("k1_emit file: ok");
    return 0;
  }
  file_checks(false);
  const uint32_t strides[] = {1, 2, 3, 4, 5, 7, 8, 9, 64, 4096, 5000, 1u << 23, 0x7fffffffu};
  const uint32_t S = (uint32_t)rpt::kStageSlots;
  for (uint32_t stride : strides) {
    run_file("empty file", {0, 0, 0}, stride);
    run_file("one sample", {0, 1, 0}, stride);
    run_file("k mod 7 rows", {0 + 1 + 2 + 3, 4 + 5 + 6 + 0, 1 + 2 + 3 + 4, 5 + 6 + 0 + 1, 2}, stride);
    run_file("full groups", {4096, 4096, 4096, 1024}, stride);
    // the staging edge: S and S + 1 outputs from one kept count, after 0 .. stride-1 (or 7)
    // samples of a group before it
    for (uint32_t before = 0; before < 8 && before < stride + 1; ++before) {
      if ((uint64_t)S * stride + 1 > 4096) break;
      run_file("edge", {before, S * stride + 1, 3}, stride);
      run_file("edge", {before, S * stride, 3}, stride);
      run_file("edge", {before, (S - 1) * stride + 1, 3}, stride);
    }
    for (int rep = 0; rep < 300; ++rep) {
      std::vector<uint32_t> g;
      const int n = 1 + (int)(rnd() % 30u);
      for (int k = 0; k < n; ++k)
        g.push_back(rnd() % 4u == 0u ? 0u : (rnd() % 8u == 0u ? rnd() % 4097u : rnd() % 90u));
      run_file("random", g, stride);
    }
  }
  // the last group of the largest file: rank + total = 2^32 - 1, every stride
  for (uint32_t stride : strides) {
    const rpt::EmitStride es = rpt::emit_stride(stride);
    const uint32_t total = 4096, rank = 0xffffffffu - total;
    const rpt::EmitSpan sp = rpt::emit_span(rank, total, es);
    const uint64_t first = ((uint64_t)rank + stride - 1) / stride;
    const uint64_t last = ((uint64_t)rank + total + stride - 1) / stride;
    CHECK(sp.first == first && sp.m == last - first, "2^32 - 1: stride %u", stride);
    CHECK(sp.m == 0 || sp.rank0 == first * stride - rank, "2^32 - 1: stride %u rank0", stride);
  }
  if (g_fail) {
    std::fprintf(stderr, "k1_emit: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("k1_emit: ok");
  return 0;
}
