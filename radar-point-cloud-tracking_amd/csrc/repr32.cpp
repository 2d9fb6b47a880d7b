// rpt_float32_repr: the device formatter's per-value routine (repr32.h) on the host, no GPU
// involved.  Kept free of HIP so that it also compiles as plain C++ (tools/asan/repr32_main.cpp).
#include <cstring>

#include "repr32.h"
#include "rpt.h"

extern "C" int32_t rpt_float32_repr(const float* v, int64_t n, char* out, int32_t* len) {
  if (n < 0 || (n > 0 && (!v || !out || !len))) return RPT_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    uint32_t bits;
    std::memcpy(&bits, v + i, sizeof(bits));
    char* slot = out + i * RPT_FLOAT32_REPR_SLOT;
    std::memset(slot, 0, RPT_FLOAT32_REPR_SLOT);
    rpt::repr32::Dec d;
    if (!rpt::repr32::decimal(bits, &d)) {
      len[i] = 0;
      continue;
    }
    const int want = rpt::repr32::length(d);
    uint8_t* end = rpt::repr32::put(reinterpret_cast<uint8_t*>(slot), d);
    // length() and put() are the two halves the kernels rely on agreeing: -1 when they do not
    len[i] = (end - reinterpret_cast<uint8_t*>(slot)) == want ? want : -1;
  }
  return RPT_OK;
}
