// rpt_grid64_plan / rpt_grid64_index: the grid rule of rpt_stdbscan_f64 (grid64.h) behind the
// C ABI, for tests without a GPU.  Host-only (see host_common.h).
#include "grid64.h"

#include "host_common.h"

extern "C" int32_t rpt_grid64_plan(const double* lo4, const double* hi4, int64_t n_finite_t,
                                   int32_t dim, double eps_space, double eps_time, int64_t n,
                                   rpt_grid64* out) {
  rpt::clear_error();
  if (!lo4 || !hi4 || !out || (dim != 2 && dim != 3) || n < 1 || !(eps_space >= 0.0) ||
      !(eps_time >= 0.0)) {
    rpt::set_error("rpt_grid64_plan: bad arguments");
    return RPT_EINVAL;
  }
  const rpt::Grid64 g = rpt::grid64_plan(lo4, hi4, n_finite_t, dim, eps_space, eps_time, n);
  for (int k = 0; k < 4; ++k) out->lo[k] = g.lo[k];
  out->cs = g.cs;
  out->ct = g.ct;
  out->dims[0] = g.nx;
  out->dims[1] = g.ny;
  out->dims[2] = g.nz;
  out->dims[3] = g.nt;
  out->cells = g.cells;
  out->doublings = g.doublings;
  out->collapsed = g.collapsed;
  return RPT_OK;
}

extern "C" int32_t rpt_grid64_index(double v, double lo, double side, int32_t n) {
  return rpt::grid64_index(v, lo, side, n);
}
