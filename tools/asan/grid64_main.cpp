// Stand-alone AddressSanitizer + UBSan program over the grid rule of the float64 ST-DBSCAN
// (csrc/grid64.h, plain C++ shared with the kernels): grid64_plan and grid64_index over the
// extremes -- extents of 1e300, eps of 1e-300 and denormal, zero extent, n = 1, infinite and zero
// eps_time, the cases that need more than 200 doublings and those that exhaust the loop (an
// extent that is not finite) -- and over random parameters.  Every plan must stay within the
// cell cap with dims >= 1 (UBSan watches the double -> integer conversions), and every index
// within its axis; on each planned grid, values one rounded eps apart must land in cells that
// differ by at most one.
//   make -C tools/asan grid64
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "grid64.h"

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
double rnd01() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) / 9007199254740992.0;
}

const double kInf = std::numeric_limits<double>::infinity();

rpt::Grid64 run_case(const char* name, const double lo[4], const double hi[4], int64_t nft,
                     int dim, double eps, double et, int64_t n) {
  const rpt::Grid64 g = rpt::grid64_plan(lo, hi, nft, dim, eps, et, n);
  const int64_t cap = rpt::grid64_cell_cap(n);
  CHECK(g.nx >= 1 && g.ny >= 1 && g.nz >= 1 && g.nt >= 1, "%s: dims", name);
  CHECK(g.cells >= 1 && g.cells <= cap, "%s: cells %lld > cap %lld", name, (long long)g.cells,
        (long long)cap);
  CHECK(g.cells == (int64_t)g.nx * g.ny * g.nz * g.nt, "%s: product", name);
  CHECK(dim == 3 || g.nz == 1, "%s: nz in 2-D", name);
  CHECK(g.cs > 0.0 && g.ct > 0.0, "%s: sides", name);
  if (eps > 0.0 && std::isfinite(g.cs)) CHECK(g.cs > eps, "%s: cell side lost its margin", name);
  if (et > 0.0 && std::isfinite(g.ct)) CHECK(g.ct > et, "%s: slab width lost its margin", name);
  // the values of the box and beyond stay inside the axis
  const double probe[] = {0.0, 0.25, 0.5, 1.0, -0.5, 1.5};
  const int32_t dims[4] = {g.nx, g.ny, g.nz, g.nt};
  for (int k = 0; k < 4; ++k) {
    const double side = k < 3 ? g.cs : g.ct;
    for (double f : probe) {
      const double v = lo[k] + f * (hi[k] - lo[k]);
      const int32_t i = rpt::grid64_index(v, g.lo[k], side, dims[k]);
      CHECK(i >= 0 && i < dims[k], "%s: index %d of axis %d", name, i, k);
    }
    for (double v : {kInf, -kInf, std::nan(""), 1.7e308, -1.7e308}) {
      const int32_t i = rpt::grid64_index(v, g.lo[k], side, dims[k]);
      CHECK(i >= 0 && i < dims[k], "%s: index of a special value", name);
    }
    CHECK(rpt::grid64_index(hi[k], g.lo[k], side, dims[k]) <= dims[k] - 1, "%s: hi", name);
  }
  // neighbours by the rounded test are at most one cell apart (x axis, uncollapsed grids)
  if (eps > 0.0 && std::isfinite(g.cs) && std::isfinite(hi[0] - lo[0])) {
    const double eps2 = eps * eps;
    for (int r = 0; r < 64; ++r) {
      const double a = lo[0] + rnd01() * (hi[0] - lo[0]);
      for (double b : {a + eps, std::nextafter(a + eps, kInf), std::nextafter(a + eps, -kInf)}) {
        if (!(b <= hi[0])) continue;
        const double d = a - b;
        if (!(d * d <= eps2)) continue;
        const int32_t ia = rpt::grid64_index(a, g.lo[0], g.cs, g.nx);
        const int32_t ib = rpt::grid64_index(b, g.lo[0], g.cs, g.nx);
        CHECK(ib - ia <= 1 && ia - ib <= 1, "%s: neighbours %d cells apart", name, ib - ia);
      }
    }
  }
  return g;
}

}  // namespace

int main() {
  {
    const double lo[4] = {0, 0, 0, 0}, hi[4] = {1e300, 1e300, 1e300, 1e300};
    const rpt::Grid64 g = run_case("extent 1e300", lo, hi, 10, 3, 1.0, 1.0, 10);
    CHECK(g.doublings > 200 && g.collapsed == 0, "extent 1e300: %d doublings", g.doublings);
  }
  {
    const double lo[4] = {-1e300, 0, 0, 0}, hi[4] = {1e300, 1.0, 0, 5.0};
    const rpt::Grid64 g = run_case("eps 1e-300", lo, hi, 10, 2, 1e-300, 0.5, 1000);
    CHECK(g.doublings > 200 && g.collapsed == 0, "eps 1e-300: %d doublings", g.doublings);
  }
  {
    const double lo[4] = {0, 0, 0, 0}, hi[4] = {1.0, 1.0, 1.0, 1.0};
    run_case("denormal eps", lo, hi, 5, 3, 5e-324, 5e-324, 5);
    const double hd[4] = {1e-310, 1e-310, 0, 1e-310};
    run_case("denormal everything", lo, hd, 5, 2, 1e-315, 1e-315, 5);
  }
  {
    const double p[4] = {3.5, -2.0, 7.0, 1.7e9};
    const rpt::Grid64 g = run_case("zero extent", p, p, 4, 3, 0.3, 0.5, 4);
    CHECK(g.cells == 1, "zero extent: one cell");
    const rpt::Grid64 g1 = run_case("n = 1", p, p, 1, 2, 0.3, 1.0, 1);
    CHECK(g1.cells == 1, "n = 1: one cell");
  }
  {
    const double lo[4] = {0, 0, 0, 0}, hi[4] = {100.0, 100.0, 0, 1e9};
    const rpt::Grid64 gi = run_case("eps_t inf", lo, hi, 50, 2, 1.0, kInf, 50);
    CHECK(gi.nt == 1, "eps_t inf: one slab");
    const rpt::Grid64 g0 = run_case("eps_t 0", lo, hi, 50, 2, 1.0, 0.0, 50);
    CHECK(g0.nt >= 1, "eps_t 0");
    const double h3[4] = {100.0, 100.0, 50.0, 10.0};
    const double hs[4] = {10.0, 10.0, 5.0, 10.0};
    const rpt::Grid64 ge = run_case("eps 0", lo, hs, 50, 3, 0.0, 1.0, 50);
    CHECK(ge.doublings == 0 && ge.nx == 11 && ge.nz == 6, "eps 0: side 1");
    run_case("eps inf", lo, h3, 50, 3, kInf, 1.0, 50);
    run_case("eps near DBL_MAX", lo, h3, 50, 3, 1.7976931348623157e308, 1.7976931348623157e308,
             50);
  }
  {  // the loop runs out: extents that are not finite
    const double lo[4] = {-1.7e308, 0, 0, 0}, hi[4] = {1.7e308, 1.0, 0, 1.0};
    const rpt::Grid64 g = run_case("x overflows", lo, hi, 9, 2, 1.0, 1.0, 9);
    CHECK(g.doublings == rpt::kGrid64Doublings && g.collapsed == 1, "x overflows: collapsed %d",
          g.collapsed);
    const double lt[4] = {0, 0, 0, -1.7e308}, ht[4] = {1.0, 1.0, 0, 1.7e308};
    const rpt::Grid64 gt = run_case("t overflows", lt, ht, 9, 2, 1.0, 1.0, 9);
    CHECK(gt.collapsed == 3 && gt.cells == 1, "t overflows: collapsed %d", gt.collapsed);
    const double la[4] = {-1.7e308, -1.7e308, -1.7e308, -1.7e308};
    const double ha[4] = {1.7e308, 1.7e308, 1.7e308, 1.7e308};
    run_case("everything overflows", la, ha, 9, 3, 1e-300, 1e-300, (int64_t(1) << 31) - 3);
  }
  {  // no finite time: hi < lo as the bounds kernel leaves them
    const double lo[4] = {0, 0, 0, kInf}, hi[4] = {1.0, 1.0, 0, -kInf};
    const rpt::Grid64 g = run_case("no finite time", lo, hi, 0, 2, 1.0, 1.0, 9);
    CHECK(g.nt == 1 && g.lo[3] == 0.0, "no finite time: one slab at 0");
  }
  for (int rep = 0; rep < 20000; ++rep) {
    double lo[4], hi[4];
    for (int k = 0; k < 4; ++k) {
      lo[k] = (rnd01() - 0.5) * std::pow(10.0, rnd01() * 600.0 - 300.0);
      hi[k] = lo[k] + rnd01() * std::pow(10.0, rnd01() * 600.0 - 300.0);
    }
    const double eps = rnd01() < 0.05 ? 0.0 : std::pow(10.0, rnd01() * 640.0 - 323.0);
    const double et = rnd01() < 0.05 ? (rnd01() < 0.5 ? 0.0 : kInf)
                                     : std::pow(10.0, rnd01() * 640.0 - 323.0);
    const int64_t n = 1 + (int64_t)(rnd01() * rnd01() * 2147483000.0);
    run_case("random", lo, hi, n, rnd01() < 0.5 ? 2 : 3, eps, et, n);
  }
  if (g_fail) {
    std::fprintf(stderr, "grid64: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::puts("grid64: ok");
  return 0;
}
