// stdbscan64.hip, what every stage reads: the launch geometry, the device form of the grid, the
// exact pair test and the window walk.  No kernel.  Included inside namespace rpt { namespace {.

constexpr int kBlock = 256;
// lanes per point in the window passes: a group of kLanes lanes strides over one point's
// candidates, four points per wave
constexpr int kLanes = 16;
constexpr int kPtsPerBlock = kBlock / kLanes;
// grid caps (blocks); above them the kernels stride
constexpr int kCapPoint = 2048;   // one thread per point: strides above 524,288 points
constexpr int kCapCell = 2048;    // one thread per cell: strides above 524,288 cells
constexpr int kCapBounds = 1024;  // bounds partials: strides above 262,144 points
constexpr int kCapWalk = 65536;   // kLanes lanes per point: strides above 1,048,576 points

// the grid as the kernels read it (Grid64, grid64.h) with the pair test's constants
struct Geom64 {
  double ox, oy, oz, ot;
  double cs, ct;
  double eps2;    // eps_space^2, rounded once
  double epst;    // float64 times: eps_time
  float epst32;   // float32 times: eps_time rounded to float32
  int32_t nx, ny, nz, nt;
  int32_t cells;  // <= 2^30; the isolated cell (points with a non-finite time) is number `cells`
  int32_t min_samples;
};

// the sorted points: structure of arrays in cell order, times widened to double (exact)
struct Pts64 {
  const double* __restrict__ x;
  const double* __restrict__ y;
  const double* __restrict__ z;  // null in 2-D
  const double* __restrict__ t;
};

// one point's values, read once by every lane of its group
struct P64 {
  double x, y, z, t;
};

template <int D>
__device__ __forceinline__ P64 load_pt(const Pts64& p, int i) {
  P64 v;
  v.x = p.x[i];
  v.y = p.y[i];
  v.z = D == 3 ? p.z[i] : 0.0;
  v.t = p.t[i];
  return v;
}

// the neighbour predicate of the contract (stdbscan64.h); this unit compiles with contraction
// off, so each operation below is rounded on its own
template <int D, bool TF64>
__device__ __forceinline__ bool near64(const P64& a, const P64& b, const Geom64& g) {
  const double dx = a.x - b.x, dy = a.y - b.y;
  double d2 = dx * dx + dy * dy;
  if (D == 3) {
    const double dz = a.z - b.z;
    d2 = d2 + dz * dz;
  }
  bool tn;
  if (TF64) {
    tn = fabs(b.t - a.t) <= g.epst;
  } else {
    tn = fabsf((float)b.t - (float)a.t) <= g.epst32;  // (the casts are exact: widened floats)
  }
  return d2 <= g.eps2 && tn;
}

__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kLanes);
  return v;
}
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
  for (int off = kLanes / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kLanes));
  return v;
}

// The window of a point in cell `cell` (< g.cells): its 3 slabs x 3 rows (x 3 layers), clipped
// at the grid's faces.  In each the x cells cx-1 .. cx+1, clipped at the row's ends, are
// consecutive cell numbers, so their points are one range [b, e) of the sorted order: 9 (27)
// ranges.  range(b, e) is called for each non-empty one by every lane of the group and returns
// false to end the walk; its result must be the same in every lane of the group.
template <int D, class F>
__device__ __forceinline__ void walk64(const Geom64& g, const int32_t* __restrict__ cell_start,
                                       int cell, F&& range) {
  const int cx = cell % g.nx;
  int r = cell / g.nx;
  const int cy = r % g.ny;
  r /= g.ny;
  const int cz = r % g.nz;
  const int ct = r / g.nz;
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
  for (int t = max(ct - 1, 0); t <= min(ct + 1, g.nt - 1); ++t)
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
      for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
        const int row = ((t * g.nz + z) * g.ny + y) * g.nx;  // < cells <= 2^30
        const int b = cell_start[row + x0], e = cell_start[row + x1 + 1];
        if (b < e && !range(b, e)) return;
      }
}
