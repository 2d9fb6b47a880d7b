// K1: polar -> Cartesian scatter with intensity threshold, per-file stride and gain fusion.
// Replaces load_radar_csv (PointCloudWork/4_temporal_object_tracker.py:200-232) + build_frame's
// concatenation (:312-352), and radar_pipeline sweep_to_point_cloud (core/transforms.py:37-79).
//
// Layout: echo [file][row][bin] (u8 — 1 B per echo sample, the radar's native 8-bit values — or
// f32), rows of 1024 bins.  One wave owns one row: with u8 echo a row is exactly one 16-B-per-lane
// coalesced load (1 KiB per wave instruction); f32 rows take four.  Kept elements are ranked in
// row-major order with a wave prefix sum over per-lane counts; the file rank comes from the
// row prefix written by the count pass (two reads of the echo, no atomics, deterministic).
//
// Arithmetic (each op rounded to float32, no contraction — the reference is separate numpy ufuncs):
//   step = scale[row] / (float)bins ; r = step * (float)bin ; x = r * cos_t[row] ; y = r * sin_t[row]
// cos_t / sin_t are inputs: numpy's float32 SIMD cos/sin are not correctly rounded, so the host
// evaluates them exactly as the reference does (4096 values per sweep geometry).
//
// This file is the one translation unit: the rule that picks the grouped u8 kernels, the host
// driver (count_impl, write_impl) and the C-ABI bodies.  Every kernel and device helper is in a
// stage file, included (inside namespace rpt { namespace {) in this order; a stage file reads
// polar_shared.inc and no other stage file.  Each file's header names the host function that
// launches its kernels, what they read and what they leave behind for the next stage.
//   polar_shared.inc  what more than one stage or the driver reads (and k_bounds_parts)
//   polar_rows.inc    generic per-row K1: k_row_count, k_file_counts, k_row_write
//   polar_count.inc   grouped u8 count pass, both staging layouts; count_waves_per_file
//   polar_write.inc   grouped u8 write pass, one wave per group: k_group_write_u8
//   polar_expand.inc  writes from staged entries: k_group_starts + k_expand_write (by rank),
//                     k_file_staged + k_expand_stream (file-contiguous)
//   polar_aux.inc     frame times / fill, bytes to float, dense polar, colours, synthetic echo
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "dispatch.h"  // with_bool, with_waves
#include "k1_emit.h"
#include "polar.h"

#pragma clang fp contract(off)

namespace rpt {
namespace {

#include "polar_shared.inc"
#include "polar_rows.inc"
#include "polar_count.inc"
#include "polar_write.inc"
#include "polar_expand.inc"
#include "polar_aux.inc"

// integer threshold of u8 samples (see keep_bits)
inline int u8_threshold(float thr) {
  if (!(thr == thr)) return 255;
  const double f = std::floor((double)thr);
  return f < -1.0 ? -1 : (f > 255.0 ? 255 : (int)f);
}

template <class T>
constexpr bool is_u8() { return false; }
template <>
constexpr bool is_u8<uint8_t>() { return true; }

// The grouped u8 kernels take u8 sweeps of exactly 1024 bins with 16-B aligned rows; row_prefix
// then holds the per-GROUP exclusive prefix (n_files * ceil(rows / 4) + 1 values), otherwise the
// per-row one.  Count and write decide the same way from the same arguments.
template <class T>
bool grouped_u8(const T* echo, int bins) {
  return is_u8<T>() && bins == 1024 && (uintptr_t)echo % 16 == 0;
}

inline uint32_t u8_k(int T) {
  return (uint32_t)(T <= 127 ? 127 - T : 255 - T) * 0x01010101u;
}

// k_expand_write and k_expand_stream: a persistent grid (8 blocks per CU of the 256; each walks a
// contiguous tile range).  ab().k1_expand off keeps the wave-per-group write for A/B runs.
constexpr int kExpandBlocks = 2048;
constexpr int kListBlocks = 2048;  // blocks of the unstaged groups' write (at most)

template <class T>
int32_t count_impl(const T* echo, int64_t n_files, int rows, int bins, float thr, int stride,
                   int64_t* row_prefix, int64_t* file_offsets, int64_t* total_host,
                   hipStream_t st, uint32_t* entries = nullptr) {
  const int64_t n_rows = n_files * rows;
  if ((int64_t)rows * bins >= (int64_t(1) << 32) || n_rows >= (int64_t(1) << 32)) {
    set_error("rpt_polar_count: rows*bins and n_files*rows must be < 2^32");
    return RPT_ENOTSUP;
  }
  const bool grouped = grouped_u8(echo, bins);
  const GroupMap gm{(uint32_t)((rows + kGroupRows - 1) / kGroupRows), rows};
  const int64_t n_units = grouped ? n_files * (int64_t)gm.gpf : n_rows;
  Scratch& sc = scratch(st);
  Budget b;
  b.add<int32_t>(n_units);
  b.add<int64_t>(n_files);
  RPT_TRY(sc.reserve(b.bytes, st));
  int32_t* rc = sc.carve_n<int32_t>(n_units);
  int64_t* fo = sc.carve_n<int64_t>(n_files);
  const bool vec = (bins % (64 * Vec<T>::N) == 0) && ((uintptr_t)echo % 16 == 0);
  const int grid = grid_for(n_units, kWavesPerBlock, 16384);
  if (grouped) {
    const int T8 = u8_threshold(thr);
    const auto* e8 = reinterpret_cast<const uint8_t*>(echo);
    const bool hi = !(T8 <= 127);  // keep_bits<HI>
    if (entries && staged_emitted(n_files, rows)) {
      // one workgroup of W waves per file (n_files < 2^32 / rows: a valid grid size)
      with_waves(count_waves_per_file(n_files), [&](auto w) {
        with_bool(hi, [&](auto h) {
          constexpr int W = decltype(w)::value;
          hipLaunchKernelGGL((k_group_count_u8_files<decltype(h)::value, W>),
                             dim3((unsigned)n_files), dim3(64 * W), 0, st, e8, gm, u8_k(T8),
                             emit_stride((uint32_t)stride), rc, entries);
        });
      });
    } else {
      with_bool(entries != nullptr, [&](auto stage) {
        with_bool(hi, [&](auto h) {
          hipLaunchKernelGGL((k_group_count_u8<decltype(h)::value, decltype(stage)::value>),
                             dim3(grid), dim3(kBlock), 0, st, e8, (uint32_t)n_units, gm, u8_k(T8),
                             rc, entries, stride == 4 ? 1 : 0);
        });
      });
    }
  } else {
    with_bool(vec, [&](auto vc) {
      hipLaunchKernelGGL((k_row_count<T, decltype(vc)::value>), dim3(grid), dim3(kBlock), 0, st,
                         echo, n_rows, bins, thr, rc);
    });
  }
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i32_to_i64(rc, row_prefix, n_units, st));
  if (grouped)
    hipLaunchKernelGGL(k_file_counts_groups, dim3(grid_for(n_files, 256, 1024)), dim3(256), 0, st,
                       row_prefix, n_files, gm.gpf, stride, fo);
  else
    hipLaunchKernelGGL(k_file_counts, dim3(grid_for(n_files, 256, 1024)), dim3(256), 0, st,
                       row_prefix, n_files, rows, stride, fo);
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i64(fo, file_offsets, n_files, st));
  if (total_host) {
    RPT_HIP(hipMemcpyAsync(total_host, file_offsets + n_files, sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
  }
  return RPT_OK;
}

template <class T, class VT = float>
int32_t write_impl(const T* echo, int64_t n_files, int rows, int bins, float thr, int stride,
                   RowGeo geo, const int32_t* gain, const int64_t* row_prefix,
                   const int64_t* file_offsets, int fpf, float* x, float* y, VT* v,
                   int32_t* gout, int32_t* pf, hipStream_t st, int64_t cap = INT64_MAX,
                   const uint32_t* entries = nullptr, uint32_t* bnd = nullptr,
                   bool* bnd_done = nullptr) {
  // bnd (nullable; polar_bounds_words() words): on the expand-write path the written points' xy
  // bounds land in bnd[0..3] (ordered u32, as k_bounds_xy) and *bnd_done is set
  if (bnd_done) *bnd_done = false;
  const int64_t n_rows = n_files * rows;
  if ((int64_t)rows * bins >= (int64_t(1) << 32) || n_rows >= (int64_t(1) << 32) || stride < 1 ||
      fpf < 1) {
    set_error("rpt_polar_write: rows*bins and n_files*rows must be < 2^32, stride/fpf >= 1");
    return RPT_ENOTSUP;
  }
  const bool vec = (bins % (64 * Vec<T>::N) == 0) && ((uintptr_t)echo % 16 == 0);
  if (grouped_u8(echo, bins) && geo.scale) {
    const GroupMap gm{(uint32_t)((rows + kGroupRows - 1) / kGroupRows), rows};
    const int64_t n_groups = n_files * (int64_t)gm.gpf;
    const int grid = grid_for(n_groups, kWavesPerBlock, 16384);
    const int T8 = u8_threshold(thr);
    const auto* e8 = reinterpret_cast<const uint8_t*>(echo);
    const bool emitted = staged_emitted(n_files, rows);  // the entries' layout, as the count pass
    // k_group_write_u8<HI, STAGED, LIST, VT> over `blocks` blocks; the callers below never ask
    // for STAGED with LIST (that form does not exist)
    auto group_write = [&](auto staged, auto listed, int blocks, const uint32_t* list,
                           const uint32_t* list_n, uint32_t* bpart) {
      with_bool(!(T8 <= 127), [&](auto h) {
        hipLaunchKernelGGL((k_group_write_u8<decltype(h)::value, decltype(staged)::value,
                                             decltype(listed)::value, VT>),
                           dim3(blocks), dim3(kBlock), 0, st, e8, (uint32_t)n_groups, gm, u8_k(T8),
                           stride, geo.scale, geo.cos_t, geo.sin_t, gain, row_prefix, file_offsets,
                           fpf, x, y, v, gout, pf, cap, entries, emitted, list, list_n, bpart);
      });
    };
    if (entries && ab().k1_expand &&
        (emitted || (stride < (1 << 23) &&
                     n_files * (int64_t)rows * 1024 < (int64_t(1) << kGsBits)))) {
      // staged entries: outputs to threads.  File-contiguous: k_file_staged + k_expand_stream;
      // by rank: k_group_starts + k_expand_write.  The few unstaged groups that the first kernel
      // of either pair lists are written by the wave-per-group kernel
      Scratch& sc = scratch(st);
      Budget b;
      if (emitted)
        b.add<uint32_t>(n_files);
      else
        b.add<uint64_t>(n_groups);
      b.add<uint32_t>(n_groups);
      RPT_TRY(sc.reserve(b.bytes, st));
      uint64_t* gword = emitted ? nullptr : sc.carve_n<uint64_t>(n_groups);
      uint32_t* staged_out = emitted ? sc.carve_n<uint32_t>(n_files) : nullptr;
      uint32_t* list = sc.carve_n<uint32_t>(n_groups);
      uint32_t* list_n = nullptr;
      RPT_TRY(zero_n(st, 1, &list_n));
      if (emitted)
        hipLaunchKernelGGL(k_file_staged, dim3(grid_for(n_files, kWavesPerBlock)), dim3(kBlock), 0,
                           st, row_prefix, file_offsets, (uint32_t)n_files, gm.gpf,
                           (uint32_t)stride, staged_out, list, list_n);
      else
        hipLaunchKernelGGL(k_group_starts, dim3(grid_for(n_groups, kBlock, 4096)), dim3(kBlock), 0,
                           st, row_prefix, file_offsets, (uint32_t)n_groups, gm.gpf,
                           (uint32_t)stride, gword, list, list_n);
      RPT_CHECK_LAUNCH();
      auto al16 = [](const void* q) { return ((uintptr_t)q & 15u) == 0; };
      const bool vec4 = al16(x) && al16(y) && al16(v) && (!gout || al16(gout)) && (!pf || al16(pf));
      const uint32_t estep = stride == 4 ? 1u : (uint32_t)stride;
      uint32_t* bpart = bnd ? bnd + 4 : nullptr;
      if (emitted)
        with_bool(vec4, [&](auto vc) {
          hipLaunchKernelGGL((k_expand_stream<decltype(vc)::value, VT>), dim3(kExpandBlocks),
                             dim3(kBlock), 0, st, file_offsets, (uint32_t)n_files, staged_out, gm,
                             geo.scale, geo.cos_t, geo.sin_t, gain, fpf, x, y, v, gout, pf, cap,
                             entries, bpart);
        });
      else
        with_bool(vec4, [&](auto vc) {
          hipLaunchKernelGGL((k_expand_write<decltype(vc)::value, VT>), dim3(kExpandBlocks),
                             dim3(kBlock), 0, st, gword, (uint32_t)n_groups, gm, estep, geo.scale,
                             geo.cos_t, geo.sin_t, gain, file_offsets + n_files, fpf, x, y, v, gout,
                             pf, cap, entries, bpart);
        });
      RPT_CHECK_LAUNCH();
      const int lgrid = std::min(grid, kListBlocks);
      group_write(std::false_type{}, std::true_type{}, lgrid, list, list_n,
                  bnd ? bnd + 4 + 4 * kExpandBlocks : nullptr);
      if (bnd) {
        hipLaunchKernelGGL(k_bounds_parts, dim3(1), dim3(kBlock), 0, st, bnd + 4,
                           kExpandBlocks + lgrid, bnd);
        if (bnd_done) *bnd_done = true;
      }
      RPT_CHECK_LAUNCH();
      return RPT_OK;
    }
    // the wave-per-group write of every group (list, list_n, bpart: the kernel's defaults)
    with_bool(entries != nullptr, [&](auto staged) {
      group_write(staged, std::false_type{}, grid, nullptr, nullptr, nullptr);
    });
  } else if (cap != INT64_MAX) {
    set_error("rpt_polar_write: a capacity-bounded write needs u8 sweeps of 1024 bins");
    return RPT_ENOTSUP;
  } else if (grouped_u8(echo, bins)) {
    set_error("rpt_polar_write: u8 sweeps take per-row scale geometry");
    return RPT_ENOTSUP;
  } else if constexpr (sizeof(VT) == 1) {
    set_error("rpt_polar_write: u8 intensities need u8 sweeps of 1024 bins");
    return RPT_ENOTSUP;
  } else {  // (float intensities only: k_row_write has no VT)
    const int grid = grid_for(n_rows, kWavesPerBlock, 16384);
    with_bool(vec, [&](auto vc) {
      hipLaunchKernelGGL((k_row_write<T, decltype(vc)::value>), dim3(grid), dim3(kBlock), 0, st,
                         echo, n_rows, rows, bins, thr, stride, geo, gain, row_prefix,
                         file_offsets, fpf, x, y, v, gout, pf);
    });
  }
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

}  // namespace

// ---------------------------------------------------------------- C-ABI bodies
// grouped_u8 for the callers that hold the echo untyped: the one statement of the rule outside
// the templates (polar.h)
bool polar_grouped_u8(const void* echo, int32_t dtype, int32_t bins) {
  return dtype == RPT_ECHO_U8 && grouped_u8((const uint8_t*)echo, bins);
}

// words of the staged kept entries of rpt_polar_count / _write (u8 sweeps of 1024 bins; else 0)
int64_t polar_stage_words(int64_t n_files, int32_t rows) {
  return n_files * (int64_t)((rows + kGroupRows - 1) / kGroupRows) * kStageSlots;
}

int32_t polar_count(const void* echo, int32_t dt, int64_t n_files, int32_t rows, int32_t bins,
                    float thr, int32_t stride, int64_t* row_prefix, int64_t* file_offsets,
                    int64_t* total_host, hipStream_t st, uint32_t* entries) {
  if (!echo || n_files < 0 || rows <= 0 || bins <= 0 || stride < 1 || !row_prefix ||
      !file_offsets) {
    set_error("rpt_polar_count: bad arguments");
    return RPT_EINVAL;
  }
  if (n_files == 0) {
    RPT_HIP(hipMemsetAsync(file_offsets, 0, sizeof(int64_t), st));
    RPT_HIP(hipMemsetAsync(row_prefix, 0, sizeof(int64_t), st));
    if (total_host) *total_host = 0;
    return RPT_OK;
  }
  if (dt == RPT_ECHO_U8)
    return count_impl<uint8_t>((const uint8_t*)echo, n_files, rows, bins, thr, stride,
                               row_prefix, file_offsets, total_host, st,
                               polar_grouped_u8(echo, dt, bins) ? entries : nullptr);
  if (dt == RPT_ECHO_F32)
    return count_impl<float>((const float*)echo, n_files, rows, bins, thr, stride, row_prefix,
                             file_offsets, total_host, st);
  set_error("rpt_polar_count: unknown echo dtype %d", dt);
  return RPT_EINVAL;
}

namespace {
// The write of u8 sweeps with per-row scale geometry, the one body behind the four entry points
// below; each of them keeps its own argument checks.  VT: the intensities' type; cap: INT64_MAX
// for an unbounded write.
template <class VT>
int32_t write_u8(const uint8_t* echo, int64_t n_files, int32_t rows, int32_t bins, float thr,
                 int32_t stride, const float* scale, const float* cos_t, const float* sin_t,
                 const int32_t* gain, const int64_t* row_prefix, const int64_t* file_offsets,
                 int32_t fpf, float* x, float* y, VT* v, int32_t* gout, int32_t* pf,
                 hipStream_t st, int64_t cap, const uint32_t* entries, uint32_t* bnd,
                 bool* bnd_done) {
  RowGeo geo{scale, nullptr, cos_t, sin_t};
  return write_impl<uint8_t, VT>(echo, n_files, rows, bins, thr, stride, geo, gain, row_prefix,
                                 file_offsets, fpf, x, y, v, gout, pf, st, cap, entries, bnd,
                                 bnd_done);
}
}  // namespace

int32_t polar_write(const void* echo, int32_t dt, int64_t n_files, int32_t rows, int32_t bins,
                    const float* scale, const float* cos_t, const float* sin_t,
                    const int32_t* gain, float thr, int32_t stride, const int64_t* row_prefix,
                    const int64_t* file_offsets, int32_t fpf, float* x, float* y, float* v,
                    int32_t* gout, int32_t* pf, hipStream_t st, const uint32_t* entries,
                    uint32_t* bnd, bool* bnd_done) {
  if (bnd_done) *bnd_done = false;
  if (n_files == 0) return RPT_OK;
  if (fpf < 1) {
    set_error("rpt_polar_write: files_per_frame must be >= 1");
    return RPT_EINVAL;
  }
  if (!echo || !scale || !cos_t || !sin_t || !row_prefix || !file_offsets || !x || !y || !v ||
      stride < 1) {
    set_error("rpt_polar_write: bad arguments");
    return RPT_EINVAL;
  }
  if (dt == RPT_ECHO_U8)
    return write_u8((const uint8_t*)echo, n_files, rows, bins, thr, stride, scale, cos_t, sin_t,
                    gain, row_prefix, file_offsets, fpf, x, y, v, gout, pf, st, INT64_MAX,
                    polar_grouped_u8(echo, dt, bins) ? entries : nullptr, bnd, bnd_done);
  if (dt == RPT_ECHO_F32) {
    RowGeo geo{scale, nullptr, cos_t, sin_t};
    return write_impl<float>((const float*)echo, n_files, rows, bins, thr, stride, geo, gain,
                             row_prefix, file_offsets, fpf, x, y, v, gout, pf, st);
  }
  set_error("rpt_polar_write: unknown echo dtype %d", dt);
  return RPT_EINVAL;
}

// rpt_polar_write into outputs of capacity cap (u8 sweeps of 1024 bins): points at or beyond
// cap are dropped; the caller compares the count with cap and writes again when it overflowed.
int32_t polar_write_cap(const uint8_t* echo, int64_t n_files, int32_t rows, float thr,
                        int32_t stride, const float* scale, const float* cos_t,
                        const float* sin_t, const int32_t* gain, const int64_t* row_prefix,
                        const int64_t* file_offsets, int32_t fpf, float* x, float* y, float* v,
                        int32_t* gout, int32_t* pf, int64_t cap, hipStream_t st,
                        const uint32_t* entries, uint32_t* bnd, bool* bnd_done) {
  if (bnd_done) *bnd_done = false;
  if (!polar_grouped_u8(echo, RPT_ECHO_U8, 1024)) {
    set_error("polar_write_cap: u8 sweeps of 1024 bins with 16-B aligned rows only");
    return RPT_ENOTSUP;
  }
  return write_u8(echo, n_files, rows, 1024, thr, stride, scale, cos_t, sin_t, gain, row_prefix,
                  file_offsets, fpf, x, y, v, gout, pf, st, cap, entries, bnd, bnd_done);
}

// The same two with uint8_t intensities (the samples themselves): u8 sweeps of 1024 bins with
// 16-B aligned rows only (the stack driver's narrow path).
int32_t polar_write(const uint8_t* echo, int64_t n_files, int32_t rows, const float* scale,
                    const float* cos_t, const float* sin_t, const int32_t* gain, float thr,
                    int32_t stride, const int64_t* row_prefix, const int64_t* file_offsets,
                    int32_t fpf, float* x, float* y, uint8_t* v, int32_t* gout, int32_t* pf,
                    hipStream_t st, const uint32_t* entries, uint32_t* bnd, bool* bnd_done) {
  if (bnd_done) *bnd_done = false;
  if (n_files == 0) return RPT_OK;
  if (!polar_grouped_u8(echo, RPT_ECHO_U8, 1024) || fpf < 1 || !scale || !cos_t || !sin_t ||
      !row_prefix || !file_offsets || !x || !y || !v || stride < 1) {
    set_error("rpt_polar_write: bad arguments");
    return RPT_EINVAL;
  }
  return write_u8(echo, n_files, rows, 1024, thr, stride, scale, cos_t, sin_t, gain, row_prefix,
                  file_offsets, fpf, x, y, v, gout, pf, st, INT64_MAX, entries, bnd, bnd_done);
}

int32_t polar_write_cap(const uint8_t* echo, int64_t n_files, int32_t rows, float thr,
                        int32_t stride, const float* scale, const float* cos_t,
                        const float* sin_t, const int32_t* gain, const int64_t* row_prefix,
                        const int64_t* file_offsets, int32_t fpf, float* x, float* y, uint8_t* v,
                        int32_t* gout, int32_t* pf, int64_t cap, hipStream_t st,
                        const uint32_t* entries, uint32_t* bnd, bool* bnd_done) {
  if (bnd_done) *bnd_done = false;
  if (!polar_grouped_u8(echo, RPT_ECHO_U8, 1024)) {
    set_error("polar_write_cap: u8 sweeps of 1024 bins with 16-B aligned rows only");
    return RPT_ENOTSUP;
  }
  return write_u8(echo, n_files, rows, 1024, thr, stride, scale, cos_t, sin_t, gain, row_prefix,
                  file_offsets, fpf, x, y, v, gout, pf, st, cap, entries, bnd, bnd_done);
}

// words of the bnd buffer of polar_write / polar_write_cap: 4 + the blocks' partials
int64_t polar_bounds_words() { return 4 + 4 * (int64_t)(kExpandBlocks + kListBlocks); }

int32_t sweep_to_points(const float* inten, const float* ranges, const float* cos_t,
                        const float* sin_t, int32_t rows, int32_t bins, float thr,
                        int32_t stride, float* x, float* y, float* z, int64_t capacity,
                        int64_t* n_out_host, hipStream_t st) {
  if (!inten || !ranges || !cos_t || !sin_t || rows <= 0 || bins <= 0 || stride < 1 ||
      !n_out_host) {
    set_error("rpt_sweep_to_points: bad arguments");
    return RPT_EINVAL;
  }
  // the count pass uses the pool; keep its outputs in a second reservation-free region
  int64_t* rp = nullptr;
  int64_t* fo = nullptr;
  RPT_HIP(hipMallocAsync((void**)&rp, sizeof(int64_t) * ((int64_t)rows + 1), st));
  RPT_HIP(hipMallocAsync((void**)&fo, sizeof(int64_t) * 2, st));
  int64_t total = 0;
  int32_t s = count_impl<float>(inten, 1, rows, bins, thr, stride, rp, fo, &total, st);
  if (s == RPT_OK) {
    if (total > capacity) {
      set_error("rpt_sweep_to_points: %lld points exceed capacity %lld", (long long)total,
                (long long)capacity);
      s = RPT_EINVAL;
    } else {
      RowGeo geo{nullptr, ranges, cos_t, sin_t};
      s = write_impl<float>(inten, 1, rows, bins, thr, stride, geo, nullptr, rp, fo, 1, x, y, z,
                            nullptr, nullptr, st);
    }
  }
  (void)hipFreeAsync(rp, st);
  (void)hipFreeAsync(fo, st);
  *n_out_host = total;
  return s;
}

int32_t frame_times(const int32_t* pf, int64_t n, const int64_t* ids, float* t, hipStream_t st) {
  if (n == 0) return RPT_OK;
  hipLaunchKernelGGL(k_frame_times, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, pf, n, ids, t,
                     (const int64_t*)nullptr);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t frame_fill(const int64_t* off, int32_t n_frames, float* t, int32_t* pf, hipStream_t st) {
  if (n_frames <= 0 || (!t && !pf)) return RPT_OK;
  hipLaunchKernelGGL(k_frame_fill, dim3((unsigned)n_frames), dim3(256), 0, st, off, t, pf);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t bytes_to_float(const uint8_t* in, int64_t n, float* out, hipStream_t st) {
  if (n <= 0) return RPT_OK;
  hipLaunchKernelGGL(k_bytes_to_float, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, in, n, out);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

// n_dev: the count on the device, <= n_max
int32_t frame_times_dev(const int32_t* pf, int64_t n_max, const int64_t* n_dev, float* t,
                        hipStream_t st) {
  if (n_max == 0) return RPT_OK;
  hipLaunchKernelGGL(k_frame_times, dim3(grid_for(n_max, 256, 8192)), dim3(256), 0, st, pf,
                     n_max, (const int64_t*)nullptr, t, n_dev);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t polar_to_cartesian(const float* cos_t, const float* sin_t, const float* ranges,
                           int64_t rows, int64_t bins, float* x, float* y, hipStream_t st) {
  if (rows * bins == 0) return RPT_OK;
  hipLaunchKernelGGL(k_polar_dense, dim3(grid_for(rows * bins, 256, 8192)), dim3(256), 0, st,
                     cos_t, sin_t, ranges, rows, bins, x, y);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t infer_time_from_colors(const uint8_t* colors, int64_t n, const float* pal, int32_t n_pal,
                               float* out, hipStream_t st) {
  if (n == 0) return RPT_OK;
  if (n_pal <= 0) {
    set_error("attempt to get argmin of an empty sequence");
    return RPT_EINVAL;
  }
  hipLaunchKernelGGL(k_colors, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, colors, n, pal,
                     n_pal, out);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

int32_t synth_echo(const rpt_synth_params* p, int64_t frame0, int64_t n_frames,
                   const float* cos_t, const float* sin_t, const uint32_t* clutter_thresh,
                   const float* targets, const int32_t* trows, const int32_t* tbins,
                   uint8_t* echo, hipStream_t st) {
  if (!p || p->n_targets > kMaxTargets || p->rows <= 0 || p->bins <= 0 || p->n_gains <= 0) {
    set_error("rpt_synth_echo: bad parameters (n_targets <= %d)", kMaxTargets);
    return RPT_EINVAL;
  }
  const int64_t blocks = n_frames * p->n_gains * p->rows;
  if (blocks == 0) return RPT_OK;
  hipLaunchKernelGGL(k_synth, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(kBlock), 0,
                     st, *p, frame0, n_frames, cos_t, sin_t, clutter_thresh, targets, trows,
                     tbins, echo);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

}  // namespace rpt
