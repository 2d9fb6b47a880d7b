// rpt_decimal_parse_host: the device parser's per-token routine (parse32.h) on the host, no GPU
// involved.  Kept free of HIP so that it also compiles as plain C++ (tools/asan/parse32_main.cpp).
#include "parse32.h"
#include "rpt.h"

extern "C" int32_t rpt_decimal_parse_host(const char* text, const int64_t* tok_off,
                                          const int32_t* tok_len, int64_t n, float* out,
                                          uint8_t* ok) {
  if (n < 0 || (n > 0 && (!text || !tok_off || !tok_len || !out || !ok))) return RPT_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    float v = 0.0f;
    const bool in = rpt::parse32::parse(reinterpret_cast<const uint8_t*>(text) + tok_off[i],
                                        tok_len[i], &v);
    out[i] = in ? v : 0.0f;
    ok[i] = in ? 1 : 0;
  }
  return RPT_OK;
}
