// rpt_ply_records_host / rpt_ply_record_tiles: the keep rule, the colours and the 15-byte records
// of the denoise pipeline's PLY writer (plyrec.h) on the host, no GPU involved.  Kept free of HIP
// so that it also compiles as plain C++ (tools/asan/plyrec_main.cpp).
#include "plyrec.h"
#include "rpt.h"

extern "C" int64_t rpt_ply_record_tiles(int64_t n) {
  return n <= 0 ? 0 : (n + rpt::plyrec::kTile - 1) / rpt::plyrec::kTile;
}

extern "C" int64_t rpt_ply_records_host(const float* x, const float* y, const float* z,
                                        const int32_t* labels, int32_t signal_only,
                                        const uint8_t* lut, int64_t n, uint8_t* out,
                                        int64_t out_bytes, int32_t* max_label) {
  namespace pr = rpt::plyrec;
  if (n < 0 || out_bytes < 0 || (signal_only && !labels)) return -RPT_EINVAL;
  if (n > 0 && out && (!x || !y || !z || !lut)) return -RPT_EINVAL;
  if (n >= (int64_t(1) << 31)) return -RPT_ENOTSUP;
  const bool has_labels = labels != nullptr;
  int64_t kept = 0;
  int32_t mx = -1;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t lab = has_labels ? labels[i] : 0;
    if (has_labels && lab > mx) mx = lab;
    kept += pr::keep(has_labels, signal_only != 0, lab);
  }
  if (max_label) *max_label = mx;
  if (!out) return kept;
  if (kept > out_bytes / pr::kRecord) return -RPT_EINVAL;  // before a byte is written
  uint8_t* p = out;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t lab = has_labels ? labels[i] : 0;
    if (!pr::keep(has_labels, signal_only != 0, lab)) continue;
    uint32_t w[4];
    pr::words(x[i], y[i], z[i], pr::color(lut, has_labels, lab, z[i]), w);
    for (int k = 0; k < pr::kRecord; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    p += pr::kRecord;
  }
  return kept;
}
