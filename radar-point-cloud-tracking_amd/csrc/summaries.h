// The rpt:: functions that summaries.hip defines, declared once (default arguments only here).
// Included by summaries.hip itself, so every definition is compiled against its declaration, by
// abi.cpp (the extern "C" surface) and by stack_impl.h (the stack and shard drivers).
#pragma once
#include "common.h"

namespace rpt {

// radix bits of keys below v: the smallest bits >= 1 with v < 2^bits.  Label keys are label + 1,
// so n_clusters labels take radix_bits_for(n_clusters)
int radix_bits_for(int64_t v);

// K9: per-(frame, label) segments of the points [0, n) in frame-major order (pf non-decreasing):
// frame, label, count, first point index, centroid and mean intensity per segment, and each
// frame's first noise point (frame_first_noise, nullable, [n_frames]; -1 without one).  Reads the
// segment count back (*n_seg_host); a frame with more labels than the frame sort takes sends the
// call to the radix path by itself.
int32_t cluster_summaries(const int32_t* labels, const float* x, const float* y,
                          const float* inten, const int32_t* pf, int64_t n, int32_t n_frames,
                          int32_t n_clusters, int32_t* o_frame, int32_t* o_label,
                          int64_t* o_count, int64_t* o_first, float* o_cx, float* o_cy,
                          float* o_mi, int64_t* frame_first_noise, int64_t* n_seg_host,
                          hipStream_t st);
// No readback: the caller passes the radix bits and a segment-count estimate, and reads the
// count (*n_seg_dev) with its other results after one sync.  A count of -1 means a frame held
// more labels than the frame sort takes: redo with force_radix.  *radix_used tells whether the
// label bits mattered (radix path) — the frame sort takes any labels.
// frame_off (nullable; device, [n_frames + 1], frame_off[n_frames] = n): the points' frame
// offsets instead of pf, which is then not read, together with inten8, the intensities as uint8_t
// samples instead of inten (the stack driver's narrow path).
int32_t cluster_summaries_dev(const int32_t* labels, const float* x, const float* y,
                              const float* inten, const int32_t* pf, int64_t n, int32_t n_frames,
                              int bits, int64_t s_hint, int32_t* o_frame, int32_t* o_label,
                              int64_t* o_count, int64_t* o_first, float* o_cx, float* o_cy,
                              float* o_mi, int64_t* frame_first_noise,
                              const int32_t** n_seg_dev, bool force_radix, bool* radix_used,
                              hipStream_t st, const int64_t* frame_off = nullptr,
                              const uint8_t* inten8 = nullptr);
// Per-label pandas group means (count, x, y, intensity) of labels in [0, n_labels); labels
// without points keep count 0.  Synchronises once.
int32_t label_means(const int32_t* labels, const float* x, const float* y, const float* inten,
                    int64_t n, int64_t n_labels, int64_t* o_count, float* o_x, float* o_y,
                    float* o_v, hipStream_t st);

}  // namespace rpt
