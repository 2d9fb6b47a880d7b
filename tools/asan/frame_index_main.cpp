// Stand-alone AddressSanitizer + UBSan program over the narrow path's index logic
// (csrc/frame_index.h, plain C++ shared with the kernels): the frame of every point from the
// frame offsets -- by search, and per compaction tile as k_land_compact does it --
// and the kept-point offsets new_off from the tile bases as k_land_new_off_tiles does it, each
// against a brute-force restatement, over the edge cases of tests/test_stack_narrow_gpu.py.
//   make -C tools/asan frame_index
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frame_index.h"

namespace {

constexpr int kTile = 4096;  // csrc/land.hip kCompTile
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

void run_case(const char* name, const std::vector<int64_t>& counts, int tile) {
  const int32_t F = (int32_t)counts.size();
  // exactly F + 1 offsets and n flags, heap blocks of their own: a read past either end is caught
  std::vector<int64_t> off((size_t)F + 1);
  off[0] = 0;
  for (int32_t f = 0; f < F; ++f) off[(size_t)f + 1] = off[(size_t)f] + counts[(size_t)f];
  const int64_t n = off[(size_t)F];
  if (n == 0) return;
  std::vector<int32_t> want((size_t)n);
  for (int32_t f = 0; f < F; ++f)
    for (int64_t i = off[(size_t)f]; i < off[(size_t)f + 1]; ++i) want[(size_t)i] = f;
  std::vector<uint8_t> keep((size_t)n);
  for (auto& k : keep) k = (rnd() % 3u) != 0u;
  // frames: by search and per tile
  const int64_t nt = (n + tile - 1) / tile;
  for (int64_t T = 0; T < nt; ++T) {
    const int64_t lo = T * tile, hi = lo + tile < n ? lo + tile : n;
    const int32_t f0 = rpt::frame_of_point(off.data(), F, lo);
    for (int64_t i = lo; i < hi; ++i) {
      const int32_t w = want[(size_t)i];
      CHECK(rpt::frame_of_point(off.data(), F, i) == w, "%s: frame_of_point(%lld)", name,
            (long long)i);
      CHECK(rpt::frame_in_tile(off.data(), F, f0, hi, i) == w, "%s: frame_in_tile(%lld)", name,
            (long long)i);
    }
  }
  // new_off: tile bases (one entry more than tiles) + the kept points of tile T below off[f]
  std::vector<int32_t> base((size_t)nt + 1);
  base[0] = 0;
  for (int64_t T = 0; T < nt; ++T) {
    int32_t c = 0;
    for (int64_t i = T * tile; i < (T + 1) * tile && i < n; ++i) c += keep[(size_t)i];
    base[(size_t)T + 1] = base[(size_t)T] + c;
  }
  for (int32_t f = 0; f <= F; ++f) {
    int64_t T;
    int32_t r;
    rpt::new_off_split(off[(size_t)f], tile, &T, &r);
    CHECK(T >= 0 && T <= nt && r >= 0 && r < tile && T * tile + r <= n, "%s: split(%d)", name, f);
    int64_t got = base[(size_t)T];
    for (int32_t j = 0; j < r; ++j) got += keep[(size_t)(T * tile + j)];
    int64_t exp = 0;
    for (int64_t i = 0; i < off[(size_t)f]; ++i) exp += keep[(size_t)i];
    CHECK(got == exp, "%s: new_off[%d] = %lld, expected %lld", name, f, (long long)got,
          (long long)exp);
  }
}

}  // namespace

int main() {
  // empty frames: the first, two adjacent in the middle, the last
  run_case("empty frames", {0, 700, 650, 0, 0, 811, 640, 702, 0}, kTile);
  // every frame but one empty; a run of empty frames longer than a tile has points
  run_case("one built frame", {0, 0, 0, 0, 0, 0, 5000, 0, 0, 0}, kTile);
  // many tiny frames: tens of frames per tile, empty ones among them
  {
    std::vector<int64_t> c;
    for (int f = 0; f < 400; ++f) c.push_back(f % 17 == 3 ? 0 : 20 + (int64_t)(rnd() % 200u));
    run_case("tiny frames", c, kTile);
  }
  // boundaries on exact multiples of the tile, the total too
  run_case("tile edges", {kTile, 2 * kTile, 0, 100, kTile - 100, 0, kTile}, kTile);
  run_case("total on a tile edge", {1000, kTile - 1000}, kTile);
  // a whole stack smaller than one tile; a single point
  run_case("below one tile", {100, 0, 250, 3, 0, 1}, kTile);
  run_case("one point", {0, 1, 0}, kTile);
  // frames of several tiles each
  run_case("long frames", {3 * kTile + 5, 0, 2 * kTile - 5, 7}, kTile);
  // small tiles: every alignment of boundaries against tiles, at random
  for (int rep = 0; rep < 200; ++rep) {
    std::vector<int64_t> c;
    const int F = 1 + (int)(rnd() % 40u);
    for (int f = 0; f < F; ++f) c.push_back(rnd() % 4u == 0u ? 0 : (int64_t)(rnd() % 40u));
    run_case("random", c, 1 + (int)(rnd() % 16u));
  }
  if (g_fail) {
    std::fprintf(stderr, "frame_index: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("frame_index: ok");
  return 0;
}
