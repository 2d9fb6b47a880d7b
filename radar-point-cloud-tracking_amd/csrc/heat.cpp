// rpt_heat_host / rpt_fixed4_repr: the per-value routines of the gain-fusion colour kernels and
// of the "%.4f" text layout (heat.h) on the host, no GPU involved.  Kept free of HIP so that it
// also compiles as plain C++ (tools/asan/heat_main.cpp).
#include <algorithm>
#include <cstring>
#include <vector>

#include "heat.h"
#include "rpt.h"

extern "C" int32_t rpt_heat_host(const float* v, int64_t n, const int64_t* seg_off, int64_t n_seg,
                                 int32_t colors_only, float* seg_min, float* seg_p99, float* z,
                                 uint8_t* rgb) {
  if (n < 0 || (n > 0 && !v)) return RPT_EINVAL;
  if (colors_only) {
    if (n > 0 && !rgb) return RPT_EINVAL;
    for (int64_t i = 0; i < n; ++i) rpt::heat::rgb(v[i], rgb + 3 * i);
    return RPT_OK;
  }
  if (n_seg < 0 || !seg_off || seg_off[0] != 0 || seg_off[n_seg] != n) return RPT_EINVAL;
  for (int64_t s = 0; s < n_seg; ++s)
    if (seg_off[s + 1] < seg_off[s]) return RPT_EINVAL;
  std::vector<uint32_t> keys;
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t a = seg_off[s], m = seg_off[s + 1] - a;
    if (m == 0) {  // unspecified by contract; defined here
      if (seg_min) seg_min[s] = 0.0f;
      if (seg_p99) seg_p99[s] = 0.0f;
      continue;
    }
    keys.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) keys[(size_t)i] = rpt::heat::key(v[a + i]);
    int64_t lo, hi;
    float t;
    rpt::heat::rank99(m, &lo, &hi, &t);
    std::nth_element(keys.begin(), keys.begin() + lo, keys.end());
    const uint32_t klo = keys[(size_t)lo];
    // sorted[hi]: the smallest of what nth_element left behind lo
    const uint32_t khi = hi > lo ? *std::min_element(keys.begin() + lo + 1, keys.end()) : klo;
    const uint32_t kmn = *std::min_element(keys.begin(), keys.begin() + lo + 1);
    const float mn = rpt::heat::unkey(kmn);
    const float p = rpt::heat::lerp99(rpt::heat::unkey(klo), rpt::heat::unkey(khi), t);
    if (seg_min) seg_min[s] = mn;
    if (seg_p99) seg_p99[s] = p;
    for (int64_t i = a; i < a + m; ++i) {
      const float zi = rpt::heat::normalize(v[i], mn, p);
      if (z) z[i] = zi;
      if (rgb) rpt::heat::rgb(zi, rgb + 3 * i);
    }
  }
  return RPT_OK;
}

extern "C" int32_t rpt_fixed4_repr(const float* v, int64_t n, char* out, int32_t* len) {
  if (n < 0 || (n > 0 && (!v || !out || !len))) return RPT_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t bits;
    std::memcpy(&bits, v + i, sizeof(bits));
    char* slot = out + i * RPT_FIXED4_SLOT;
    std::memset(slot, 0, RPT_FIXED4_SLOT);
    rpt::fixed4::Dec d;
    if (!rpt::fixed4::decimal(bits, &d)) {
      len[i] = 0;
      continue;
    }
    const int want = rpt::fixed4::length(d);
    uint8_t* end = rpt::fixed4::put(reinterpret_cast<uint8_t*>(slot), d);
    // length() and put() are the two halves the kernels rely on agreeing: -1 when they do not
    len[i] = (end - reinterpret_cast<uint8_t*>(slot)) == want ? want : -1;
  }
  return RPT_OK;
}
