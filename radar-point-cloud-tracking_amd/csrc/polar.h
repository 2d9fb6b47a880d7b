// The rpt:: functions that polar.hip defines, declared once (default arguments only here).
// Included by polar.hip itself, so every definition is compiled against its declaration, by
// abi.cpp (the extern "C" surface) and by stack_impl.h (the stack and shard drivers).
#pragma once
#include "common.h"

namespace rpt {

// ---- K1: count pass, write pass
// The rule for the grouped u8 kernels: u8 sweeps of exactly 1024 bins with 16-B aligned rows.
// Count, write and the callers that size the staging buffer decide with it from the same
// arguments (the staging buffer and the narrow point layout exist on this condition only).
bool polar_grouped_u8(const void* echo, int32_t dtype, int32_t bins);
// words of the staged kept entries of polar_count / polar_write (grouped u8 sweeps; else unused)
int64_t polar_stage_words(int64_t n_files, int32_t rows);
// words of the bnd buffer of polar_write / polar_write_cap; the bounds they leave in bnd[0..3]
// read back as floats
int64_t polar_bounds_words();

// entries (nullable): the staging buffer, filled here and read by the write call
int32_t polar_count(const void* echo, int32_t dt, int64_t n_files, int32_t rows, int32_t bins,
                    float thr, int32_t stride, int64_t* row_prefix, int64_t* file_offsets,
                    int64_t* total_host, hipStream_t st, uint32_t* entries);
// bnd (nullable; polar_bounds_words() words): on the expand-write path the written points' xy
// bounds land in bnd[0..3] and *bnd_done is set; every form clears *bnd_done first
int32_t polar_write(const void* echo, int32_t dt, int64_t n_files, int32_t rows, int32_t bins,
                    const float* scale, const float* cos_t, const float* sin_t,
                    const int32_t* gain, float thr, int32_t stride, const int64_t* row_prefix,
                    const int64_t* file_offsets, int32_t files_per_frame, float* x, float* y,
                    float* v, int32_t* gout, int32_t* pf, hipStream_t st, const uint32_t* entries,
                    uint32_t* bnd = nullptr, bool* bnd_done = nullptr);
// polar_write into outputs of capacity cap (grouped u8 sweeps only): points at or beyond cap are
// dropped; the caller compares the count with cap and writes again when it overflowed
int32_t polar_write_cap(const uint8_t* echo, int64_t n_files, int32_t rows, float thr,
                        int32_t stride, const float* scale, const float* cos_t,
                        const float* sin_t, const int32_t* gain, const int64_t* row_prefix,
                        const int64_t* file_offsets, int32_t fpf, float* x, float* y, float* v,
                        int32_t* gout, int32_t* pf, int64_t cap, hipStream_t st,
                        const uint32_t* entries, uint32_t* bnd = nullptr,
                        bool* bnd_done = nullptr);
// the u8-intensity forms (grouped u8 sweeps only; the stack driver's narrow path): v holds the
// samples themselves
int32_t polar_write(const uint8_t* echo, int64_t n_files, int32_t rows, const float* scale,
                    const float* cos_t, const float* sin_t, const int32_t* gain, float thr,
                    int32_t stride, const int64_t* row_prefix, const int64_t* file_offsets,
                    int32_t fpf, float* x, float* y, uint8_t* v, int32_t* gout, int32_t* pf,
                    hipStream_t st, const uint32_t* entries, uint32_t* bnd = nullptr,
                    bool* bnd_done = nullptr);
int32_t polar_write_cap(const uint8_t* echo, int64_t n_files, int32_t rows, float thr,
                        int32_t stride, const float* scale, const float* cos_t,
                        const float* sin_t, const int32_t* gain, const int64_t* row_prefix,
                        const int64_t* file_offsets, int32_t fpf, float* x, float* y, uint8_t* v,
                        int32_t* gout, int32_t* pf, int64_t cap, hipStream_t st,
                        const uint32_t* entries, uint32_t* bnd = nullptr,
                        bool* bnd_done = nullptr);
int32_t sweep_to_points(const float* inten, const float* ranges, const float* cos_t,
                        const float* sin_t, int32_t rows, int32_t bins, float thr,
                        int32_t stride, float* x, float* y, float* z, int64_t capacity,
                        int64_t* n_out_host, hipStream_t st);

// ---- the small kernels beside K1 (polar_aux.inc)
int32_t frame_times(const int32_t* pf, int64_t n, const int64_t* ids, float* t, hipStream_t st);
// n_dev: the count on the device, <= n_max
int32_t frame_times_dev(const int32_t* pf, int64_t n_max, const int64_t* n_dev, float* t,
                        hipStream_t st);
// t[i] = (float)f and pf[i] = f (each nullable) for the points [off[f], off[f + 1]) of every
// frame f: frame slots from device frame offsets off[0 .. n_frames]
int32_t frame_fill(const int64_t* off, int32_t n_frames, float* t, int32_t* pf, hipStream_t st);
// out[i] = (float)in[i]
int32_t bytes_to_float(const uint8_t* in, int64_t n, float* out, hipStream_t st);
int32_t polar_to_cartesian(const float* cos_t, const float* sin_t, const float* ranges,
                           int64_t rows, int64_t bins, float* x, float* y, hipStream_t st);
int32_t infer_time_from_colors(const uint8_t* colors, int64_t n, const float* pal, int32_t n_pal,
                               float* out, hipStream_t st);
int32_t synth_echo(const rpt_synth_params* p, int64_t frame0, int64_t n_frames,
                   const float* cos_t, const float* sin_t, const uint32_t* clutter_thresh,
                   const float* targets, const int32_t* trows, const int32_t* tbins,
                   uint8_t* echo, hipStream_t st);

}  // namespace rpt
