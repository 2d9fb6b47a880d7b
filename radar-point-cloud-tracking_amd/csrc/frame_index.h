// Frame slots from frame offsets: the pure index logic of the stack driver's narrow path (no
// per-point frame array).  off[0 .. F] are non-decreasing point offsets, off[0] = 0, off[F] = n;
// point i belongs to the one frame f with off[f] <= i < off[f + 1] (empty frames repeat an
// offset and own no point).  Shared by the kernels (land.hip, summaries.hip, polar_aux.inc) and by
// the host check tools/asan/frame_index_main.cpp, so everything here is plain C++.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPT_HD __host__ __device__ __forceinline__
#else
#define RPT_HD inline
#endif

namespace rpt {

// Frame of point i in [0, off[F]): the last f in [0, F) with off[f] <= i.
RPT_HD int32_t frame_of_point(const int64_t* off, int32_t F, int64_t i) {
  int32_t lo = 0, hi = F;  // invariant: off[lo] <= i, and hi == F or off[hi] > i
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// The land compaction's per-tile form (k_land_compact<OFFS>, mirrored here for the host check):
// f0 = frame_of_point(off, F, tile_lo) once per tile, then the frame of point i in
// [tile_lo, tile_hi) is f0 + the number of offsets after off[f0] that are <= i; the walk ends at
// the first offset at or past the tile's end (off ascends).
RPT_HD int32_t frame_in_tile(const int64_t* off, int32_t F, int32_t f0, int64_t tile_hi,
                             int64_t i) {
  int32_t f = f0;
  for (int32_t q = f0 + 1; q < F; ++q) {
    const int64_t o = off[q];
    if (o >= tile_hi) break;
    f += (i >= o) ? 1 : 0;
  }
  return f;
}

// The kept-point offset of frame f after a compaction by tiles of `tile` points that keeps the
// index order: tile_base[T] + (kept points of tile T below index p), p = off[f].  Splits p into
// the tile T and the count r of tile T's leading points to look at (T may equal the tile count
// when p = n is a multiple of the tile: tile_base has one entry more than there are tiles).
RPT_HD void new_off_split(int64_t p, int32_t tile, int64_t* T, int32_t* r) {
  *T = p / tile;
  *r = (int32_t)(p - *T * tile);
}

}  // namespace rpt
