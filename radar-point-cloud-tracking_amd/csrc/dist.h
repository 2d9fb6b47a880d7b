// The rpt:: functions that dist.hip defines, declared once.  Included by dist.hip itself, so
// every definition is compiled against its declaration, by abi.cpp (the extern "C" surface) and
// by stack_impl.h (the shard driver).
#pragma once
#include "common.h"

namespace rpt {

// out[i] = the global representative of point i's component: comp[i] < 0 -> -1; otherwise
// g = base + comp[i], mapped through the sorted pairs keys[nk] -> vals[nk] where g is a key
int32_t remap_components(const int32_t* comp, int64_t n, int64_t base, const int64_t* keys,
                         const int64_t* vals, int64_t nk, int64_t* out, hipStream_t st);
// the ids base + k, lo <= k < hi, that are their own representative (rep[k] == base + k), in
// order into out; *count_host (read back) their number.  Synchronises.
int32_t select_roots(const int64_t* rep, int64_t base, int64_t lo, int64_t hi, int64_t* out,
                     int64_t* count_host, hipStream_t st);

}  // namespace rpt
