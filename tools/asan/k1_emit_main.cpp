// Stand-alone AddressSanitizer + UBSan program over K1's emission arithmetic (csrc/k1_emit.h,
// plain C++ shared with the count pass, k_group_starts and k_group_write_u8): a file's kept
// samples are cut into groups at random and every group's span (first output, output count,
// in-group rank of the first output) is checked against a brute-force walk of the file's ranks,
// for power-of-two and other strides, strides above the file's kept count, and the staging edge
// at kStageSlots under every rank residue.
//   make -C tools/asan k1_emit
// `k1_emit_main table` prints "rank total stride first m rank0 staged" for every rank < 40,
// total < 40, stride 1..9 and 64 (tests/test_k1_emit_host.py compares it with numpy).
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

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "table") == 0) return table();
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
