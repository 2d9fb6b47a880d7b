// The grid geometry of the float64 ST-DBSCAN (stdbscan64.hip): which uniform space x time grid a
// point set gets, and which cell a value falls in.  Plain C++ with no HIP header, so the rule is
// tested without a GPU (rpt_grid64_plan, tools/asan/grid64_main.cpp); stdbscan64.hip compiles the
// same two functions for the device.
//
// The rule
//   cell side   cs = max(eps, 2^-500) (1 + 2^-20); 1 for eps = 0; one cell where eps^2 overflows
//               (every pair passes d2 <= inf)
//   slab width  ct = max(eps_t, 2^-500) (1 + 2^-20); 1 for eps_t = 0; one slab for eps_t = inf
//   dims        floor(extent / side) + 1 per axis, capped at 10^9
//   cell cap    min(max(2^22, 4 n), 2^30): while the cells exceed it the larger of (slabs, cells
//               per slab) has its side doubled, as the float32 grid build does.  Up to
//               kGrid64Doublings times, which spans the exponent range of double (the float32
//               build's 200 cover float32 extents only); an extent that is not finite (hi - lo
//               overflows) still fails then, and the axes collapse to one cell: space first, then
//               time.
//   cell index  floor((v - lo) / side) in double, clamped to [0, dim - 1] (NaN -> 0)
//
// Why every neighbour lies within +-1 cell.  A pair passes the space test when the ROUNDED
// d2 <= the ROUNDED eps^2.  For eps >= 2^-500 both are normal numbers with relative error of a
// few 2^-53, so |a_k - b_k| <= eps (1 + 2^-50) on every axis; below 2^-500 the squares lose bits
// to underflow (a difference up to 2^-537 squares to zero), which is why the side never goes below
// 2^-500.  (v - lo) and the quotient are rounded once each: relative 2^-52 together, so with at
// most 2^30 cells per axis the computed position is off by less than 2^-22 cells.  Two neighbours
// are at most (1 + 2^-50) / (1 + 2^-20) < 1 - 2^-21 cells apart, their computed positions less
// than 1 - 2^-21 + 2 * 2^-22 = 1: the floors differ by at most one.  Doubling a side only
// shrinks distances in cell units.  The time axis is the same argument: the float64 test's
// t_j - t_i is rounded once (2^-53), the float32 test's once in float32 (2^-24, and exact where
// the difference is denormal), both far inside the 2^-20 margin.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RPT_GRID64_HD __host__ __device__
#else
#define RPT_GRID64_HD
#endif

namespace rpt {

constexpr int kGrid64Doublings = 2200;

struct Grid64 {
  double lo[4];    // origin of x, y, z, t (0 on an unused axis)
  double cs, ct;   // cell side, slab width (infinity on a collapsed axis)
  int32_t nx, ny, nz, nt;
  int64_t cells;   // nx * ny * nz * nt <= the cell cap; the isolated cell is number `cells`
  int32_t doublings;  // how often a side was doubled (0: the cell side is the uncoarsened one)
  int32_t collapsed;  // bit 0: space collapsed to one cell, bit 1: time too
};

inline int64_t grid64_cell_cap(int64_t n) {
  const int64_t a = int64_t(1) << 22, b = 4 * n, c = int64_t(1) << 30;
  const int64_t m = a > b ? a : b;
  return m < c ? m : c;
}

// cells along one axis of this extent; NaN (inf / inf) counts as too many
inline int64_t grid64_dim(double ext, double side) {
  const double q = std::floor(ext / side) + 1.0;
  if (!(q <= 1e9)) return (int64_t)1000000000;
  return q < 1.0 ? 1 : (int64_t)q;
}

// lo / hi: minima and maxima of the finite coordinates and the finite times (hi >= lo); dim 2
// ignores index 2.  eps_space >= 0 and eps_time >= 0 (the caller handles negative and NaN
// values), eps_time already rounded to float32 for float32 times.  n >= 1 points.
inline Grid64 grid64_plan(const double lo[4], const double hi[4], int64_t n_finite_t, int dim,
                          double eps_space, double eps_time, int64_t n) {
  Grid64 g{};
  const double margin = 1.0 + 1.0 / 1048576.0;  // 2^-20
  const double floor_side = 0x1p-500;
  for (int k = 0; k < 4; ++k) g.lo[k] = lo[k];
  double ext[4];
  for (int k = 0; k < 4; ++k) ext[k] = hi[k] - lo[k];
  if (dim != 3) {
    g.lo[2] = 0.0;
    ext[2] = 0.0;
  }
  if (n_finite_t <= 0) {
    g.lo[3] = 0.0;
    ext[3] = 0.0;
  }
  double cs = eps_space > 0.0 ? (eps_space > floor_side ? eps_space : floor_side) * margin : 1.0;
  // eps^2 overflows: d2 <= inf holds for every pair, however far apart: one cell
  if (std::isinf(eps_space * eps_space)) cs = INFINITY;
  double ct = eps_time > 0.0 ? (eps_time > floor_side ? eps_time : floor_side) * margin : 1.0;
  // (eps * margin overflows only for eps within 2^-20 of the largest double: one cell then)
  const int64_t cmax = grid64_cell_cap(n);
  int64_t nx = 1, ny = 1, nz = 1, nt = 1;
  bool fits = false;
  int it = 0;
  for (; it <= kGrid64Doublings; ++it) {
    nx = grid64_dim(ext[0], cs);
    ny = grid64_dim(ext[1], cs);
    nz = dim == 3 ? grid64_dim(ext[2], cs) : 1;
    nt = grid64_dim(ext[3], ct);
    if ((double)nx * (double)ny * (double)nz * (double)nt <= (double)cmax) {
      fits = true;
      break;
    }
    if (it == kGrid64Doublings) break;
    if ((double)nt > (double)nx * (double)ny * (double)nz)
      ct *= 2.0;
    else
      cs *= 2.0;
  }
  g.doublings = it;
  if (!fits) {  // an extent that is not finite
    cs = INFINITY;
    nx = ny = nz = 1;
    g.collapsed = 1;
    if (nt > cmax) {
      ct = INFINITY;
      nt = 1;
      g.collapsed = 3;
    }
  }
  g.cs = cs;
  g.ct = ct;
  g.nx = (int32_t)nx;
  g.ny = (int32_t)ny;
  g.nz = (int32_t)nz;
  g.nt = (int32_t)nt;
  g.cells = nx * ny * nz * nt;
  return g;
}

// the cell of v along an axis of n cells: in [0, n - 1] whatever v is
RPT_GRID64_HD inline int32_t grid64_index(double v, double lo, double side, int32_t n) {
  const double q = floor((v - lo) / side);
  if (!(q >= 1.0)) return 0;  // below the origin, the first cell, or NaN (inf / inf)
  return q < (double)n ? (int32_t)q : n - 1;
}

}  // namespace rpt
