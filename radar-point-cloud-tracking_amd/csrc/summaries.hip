// K9: per-(frame, label) cluster summaries.  Replaces the per-frame Cluster extraction of
// PointCloudWork/4_temporal_object_tracker.py:508-536 (Cluster :143-158).
//
// Pipeline: sort the points so that every (frame, label) run is contiguous and in index order,
// then summarise the runs.  The sort is a stable per-frame counting sort (one 16-wave block per
// frame, or C blocks for frames of more than 64 k points; labels hashed to LDS slots, up to
// kFsMaxKeys labels per frame) or, beyond that, a stable radix sort of (label + 1, index).  Runs
// of up to kLaneChainMax points take one lane each, longer ones two waves; the reduction orders are
// numpy's (summaries_runs.inc).  label_means shares the radix front and reduces as pandas does
// (summaries_means.inc).
//
// This file is the one translation unit: long_grid, summaries_impl (both paths), the entry points
// and label_means.  Every kernel and device helper is in a stage file, included (inside
// namespace rpt { namespace {) in this order.  Each file's header names the host function that
// launches its kernels, in what order, and what they read and leave behind.  A stage file reads
// summaries_shared.inc and no other stage file, except that the chunked sort reads the hash
// helpers and constants of summaries_fsort.inc.
//   summaries_shared.inc         kBlock, intensity loads, FramesPf / FramesOff, k_fill_i64
//   summaries_radix.inc          the kernels around the radix sort: keys, heads, starts, gather
//   summaries_runs.inc           k_runs_lane, k_summarize and numpy's reduction orders
//   summaries_means.inc          k_label_means, pandas' Kahan group mean
//   summaries_fsort.inc          k_frame_sort, k_seg_compact, k_seg_total_fix
//   summaries_fsort_chunked.inc  k_fsc_count, k_fsc_merge, k_fsc_scatter
#include <climits>
#include <cstdlib>

#include <algorithm>

#include "common.h"
#include "frame_index.h"
#include "summaries.h"

#pragma clang fp contract(off)

namespace rpt {
namespace {

#include "summaries_shared.inc"
#include "summaries_radix.inc"
#include "summaries_runs.inc"
#include "summaries_means.inc"
#include "summaries_fsort.inc"
#include "summaries_fsort_chunked.inc"

}  // namespace

// k_summarize's grid: two waves per long run, the count known only on the device (loops)
static int long_grid(int64_t s_hint) {
  return grid_for(2 * std::min<int64_t>(s_hint, 8192), kBlock / 64, 4096);
}

int radix_bits_for(int64_t v) {
  int bits = 1;
  while ((int64_t(1) << bits) <= v) ++bits;
  return bits;
}

// What the radix front leaves in the stream's scratch (summaries_radix.inc).
template <class VT>
struct RadixFront {
  uint32_t *sk, *sv;    // sorted keys (label + 1) and their point indices
  int32_t *head, *pos;  // run heads (dead after k_seg_starts) and positions; pos[n] = run count
  int64_t* seg_start;   // first sorted position of every run
  float *gx, *gy;       // the runs' points, contiguous
  VT* gi;
  int32_t* n_long;      // one more word (summaries_impl's long-run count)
};

// The radix path up to the gathered runs, for summaries_impl and label_means: reserves and carves
// the scratch, then k_sum_keys, radix_sort_pairs on `bits` bits, the caller's head kernel
// (heads(grid, sk, sv, head) launches it), exclusive_scan_total_i32, k_seg_starts and
// k_gather_runs<VT>.  With n == 0 it carves and launches nothing.
template <class VT, class Heads>
static int32_t radix_front(Scratch& sc, const int32_t* labels, const float* x, const float* y,
                           const VT* inten, int64_t n, int bits, Heads&& heads, hipStream_t st,
                           RadixFront<VT>* r) {
  Budget b;
  for (int k = 0; k < 4; ++k) b.add<uint32_t>(n + 1);
  b.add<int64_t>(radix_tmp_elems(n));
  b.add<int32_t>(n + 1);
  b.add<int32_t>(n + 1);
  b.add<int64_t>(n + 1);
  for (int k = 0; k < 3; ++k) b.add<float>(n + 1);
  b.add<int32_t>(1);
  RPT_TRY(sc.reserve(b.bytes, st));
  uint32_t* keys = sc.carve_n<uint32_t>(n + 1);
  uint32_t* vals = sc.carve_n<uint32_t>(n + 1);
  uint32_t* ka = sc.carve_n<uint32_t>(n + 1);
  uint32_t* va = sc.carve_n<uint32_t>(n + 1);
  int64_t* rtmp = sc.carve_n<int64_t>(radix_tmp_elems(n));
  r->head = sc.carve_n<int32_t>(n + 1);
  r->pos = sc.carve_n<int32_t>(n + 1);  // int32: n < 2^31 (checked by the callers)
  r->seg_start = sc.carve_n<int64_t>(n + 1);
  r->gx = sc.carve_n<float>(n + 1);
  r->gy = sc.carve_n<float>(n + 1);
  r->gi = sc.carve_n<VT>(n + 1);  // (budgeted as a float column: a u8 one needs less)
  r->n_long = sc.carve_n<int32_t>(1);
  if (n == 0) return RPT_OK;
  const int g = grid_for(n, kBlock, 8192);
  hipLaunchKernelGGL(k_sum_keys, dim3(g), dim3(kBlock), 0, st, labels, n, keys, vals);
  RPT_CHECK_LAUNCH();
  RPT_TRY(radix_sort_pairs(keys, vals, ka, va, n, bits, rtmp, &r->sk, &r->sv, st));
  heads(g, r->sk, r->sv, r->head);
  RPT_TRY(exclusive_scan_total_i32(r->head, r->pos, n, st));
  hipLaunchKernelGGL(k_seg_starts, dim3(g), dim3(kBlock), 0, st, r->head, r->pos, n,
                     r->seg_start);
  hipLaunchKernelGGL(k_gather_runs<VT>, dim3(g), dim3(kBlock), 0, st, r->sv, n, x, y, inten,
                     r->gx, r->gy, r->gi);
  return RPT_OK;
}

// bits: radix bits of the label keys (label + 1 < 2^bits); s_hint: expected segment count (sizes
// the summarize grid, which loops over the device count); *n_seg_dev: the count, on the device.
template <class FR, class VT>
static int32_t summaries_impl(const int32_t* labels, const float* x, const float* y,
                              const VT* inten, FR pf, int64_t n, int32_t n_frames,
                              int bits, int64_t s_hint, int32_t* o_frame, int32_t* o_label,
                              int64_t* o_count, int64_t* o_first, float* o_cx, float* o_cy,
                              float* o_mi, int64_t* frame_first_noise,
                              const int32_t** n_seg_dev, bool force_radix, bool* radix_used,
                              hipStream_t st) {
  if (n >= (int64_t(1) << 31) - 1) {
    set_error("rpt_cluster_summaries: n exceeds the int32 index space");
    return RPT_ENOTSUP;
  }
  Scratch& sc = scratch(st);
  // frame_first_noise = -1 (the frame-sort path clears its counters in the same launch)
  auto fill_noise = [&](int32_t* zero2) -> int32_t {
    if (n_frames > 0 && frame_first_noise) {
      hipLaunchKernelGGL(k_fill_i64, dim3(grid_for(n_frames, 256, 64)), dim3(256), 0, st,
                         frame_first_noise, (int64_t)n_frames, (int64_t)-1, zero2);
    } else if (zero2) {
      RPT_HIP(hipMemsetAsync(zero2, 0, 2 * sizeof(int32_t), st));
    }
    return RPT_OK;
  };
  const int64_t sh = std::max<int64_t>(1, std::min<int64_t>(s_hint, n));
  // per-frame counting sort unless forced off (ab().k9_radix, or a redo after a frame held more
  // than kFsMaxKeys labels) or frames are huge (one 16-wave block per frame)
  const bool frame_sort = !force_radix && !ab().k9_radix && n_frames > 0 && n > 0 &&
                          n / n_frames <= (int64_t(1) << 20);
  if (radix_used) *radix_used = !frame_sort;
  if (frame_sort) {
    // blocks per frame: one up to 64 k points per frame on average, else ~64 k points each (at
    // most 16): the dense share's 490 k-point frames take 8
    const int64_t ppf = n / std::max<int32_t>(n_frames, 1);
    const int C = (int)std::min<int64_t>(16, std::max<int64_t>(1, (ppf + 65535) / 65536));
    const int64_t NC = (int64_t)n_frames * C;
    Budget b;
    for (int k = 0; k < 3; ++k) b.add<float>(n + 1);
    for (int k = 0; k < 4; ++k) b.add<int32_t>(n + 1);
    b.add<int64_t>(n + 1);
    for (int k = 0; k < 3; ++k) b.add<int32_t>((int64_t)n_frames + 1);
    b.add<int32_t>(2);
    if (C > 1) {
      b.add<int32_t>(NC * kFsCap);
      b.add<uint32_t>(NC * kFsCap * kFsWaves);
      b.add<int32_t>(NC * kFsCap);
      b.add<int32_t>(NC * kFsCap);
      b.add<int32_t>(NC);
      b.add<int32_t>(NC);
    }
    RPT_TRY(sc.reserve(b.bytes, st));
    float* gx = sc.carve_n<float>(n + 1);
    float* gy = sc.carve_n<float>(n + 1);
    VT* gi = sc.carve_n<VT>(n + 1);  // (budgeted as a float column: a u8 one needs less)
    int32_t* tstart = sc.carve_n<int32_t>(n + 1);
    int32_t* tlen = sc.carve_n<int32_t>(n + 1);
    int32_t* tlabel = sc.carve_n<int32_t>(n + 1);
    int32_t* tfirst = sc.carve_n<int32_t>(n + 1);
    int64_t* seg_start = sc.carve_n<int64_t>(n + 1);
    int32_t* fstart = sc.carve_n<int32_t>((int64_t)n_frames + 1);
    int32_t* nseg_f = sc.carve_n<int32_t>((int64_t)n_frames + 1);
    int32_t* base = sc.carve_n<int32_t>((int64_t)n_frames + 1);
    int32_t* ovf = sc.carve_n<int32_t>(2);  // [overflow flag, long-run count]
    int32_t *ent_key = nullptr, *nent = nullptr, *fnoise_c = nullptr, *ent_base = nullptr,
            *ent_run = nullptr;
    uint32_t* ent_cnt = nullptr;
    if (C > 1) {
      ent_key = sc.carve_n<int32_t>(NC * kFsCap);
      ent_cnt = sc.carve_n<uint32_t>(NC * kFsCap * kFsWaves);
      ent_base = sc.carve_n<int32_t>(NC * kFsCap);
      ent_run = sc.carve_n<int32_t>(NC * kFsCap);
      nent = sc.carve_n<int32_t>(NC);
      fnoise_c = sc.carve_n<int32_t>(NC);
    }
    RPT_TRY(fill_noise(ovf));
    if (C == 1) {
      hipLaunchKernelGGL((k_frame_sort<FR, VT>), dim3(n_frames), dim3(kFsWaves * 64), 0, st, labels, pf, n,
                         x, y, inten, gx, gy, gi, fstart, tstart, tlen, tlabel, tfirst, nseg_f,
                         frame_first_noise, ovf);
    } else {
      hipLaunchKernelGGL(k_fsc_count<FR>, dim3((unsigned)NC), dim3(kFsWaves * 64), 0, st, labels, pf,
                         n, C, ent_key, ent_cnt, nent, fnoise_c, ovf);
      hipLaunchKernelGGL(k_fsc_merge<FR>, dim3(n_frames), dim3(kFsWaves * 64), 0, st, pf, n, C,
                         ent_key, ent_cnt, nent, fnoise_c, ent_base, ent_run, fstart, tstart,
                         tlen, tlabel, nseg_f, frame_first_noise, ovf);
      hipLaunchKernelGGL((k_fsc_scatter<FR, VT>), dim3((unsigned)NC), dim3(kFsWaves * 64), 0, st, labels,
                         pf, n, C, x, y, inten, gx, gy, gi, tfirst, ent_key, ent_cnt, nent,
                         ent_base, ent_run, ovf);
    }
    RPT_CHECK_LAUNCH();
    RPT_TRY(exclusive_scan_total_i32(nseg_f, base, n_frames, st));
    hipLaunchKernelGGL(k_seg_compact, dim3(grid_for(n_frames, 4, 1024)), dim3(256), 0, st,
                       n_frames, fstart, nseg_f, base, tstart, tlen, tlabel, tfirst, o_frame,
                       o_label, o_count, o_first, seg_start);
    hipLaunchKernelGGL(k_seg_total_fix, dim3(1), dim3(64), 0, st, ovf, base + n_frames);
    // short runs one lane each; the long ones listed (in tlen, dead after the compaction) for
    // k_summarize's waves
    hipLaunchKernelGGL((k_runs_lane<true, FR, VT>), dim3(grid_for((sh + 63) / 64, kBlock / 64, 4096)),
                       dim3(kBlock), 0, st, nullptr, nullptr, seg_start, base + n_frames, n, gx,
                       gy, gi, pf, o_frame, o_label, o_count, o_first, o_cx, o_cy, o_mi, tlen,
                       ovf + 1);
    hipLaunchKernelGGL((k_summarize<true, FR, VT>), dim3(long_grid(sh)), dim3(kBlock), 0, st, nullptr,
                       nullptr, seg_start, base + n_frames, n, gx, gy, gi, pf, o_frame, o_label,
                       o_count, o_first, o_cx, o_cy, o_mi, tlen, ovf + 1);
    RPT_CHECK_LAUNCH();
    *n_seg_dev = base + n_frames;
    return RPT_OK;
  }
  RPT_TRY(fill_noise(nullptr));
  RadixFront<VT> r;
  RPT_TRY(radix_front(
      sc, labels, x, y, inten, n, bits,
      [&](int g, const uint32_t* sk, const uint32_t* sv, int32_t* head) {
        hipLaunchKernelGGL(k_heads<FR>, dim3(g), dim3(kBlock), 0, st, sk, sv, pf, n, head,
                           frame_first_noise);
      },
      st, &r));
  if (n == 0) {
    RPT_HIP(hipMemsetAsync(r.pos, 0, sizeof(int32_t), st));
    *n_seg_dev = r.pos;
    RPT_CHECK_LAUNCH();
    return RPT_OK;
  }
  // short runs one lane each; the long ones listed (in head, dead after k_seg_starts)
  RPT_HIP(hipMemsetAsync(r.n_long, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL((k_runs_lane<false, FR, VT>), dim3(grid_for((sh + 63) / 64, kBlock / 64, 4096)),
                     dim3(kBlock), 0, st, r.sk, r.sv, r.seg_start, r.pos + n, n, r.gx, r.gy, r.gi,
                     pf, o_frame, o_label, o_count, o_first, o_cx, o_cy, o_mi, r.head, r.n_long);
  hipLaunchKernelGGL((k_summarize<false, FR, VT>), dim3(long_grid(sh)), dim3(kBlock), 0, st, r.sk,
                     r.sv, r.seg_start, r.pos + n, n, r.gx, r.gy, r.gi, pf, o_frame, o_label,
                     o_count, o_first, o_cx, o_cy, o_mi, r.head, r.n_long);
  RPT_CHECK_LAUNCH();
  *n_seg_dev = r.pos + n;
  return RPT_OK;
}

int32_t cluster_summaries(const int32_t* labels, const float* x, const float* y,
                          const float* inten, const int32_t* pf, int64_t n, int32_t n_frames,
                          int32_t n_clusters, int32_t* o_frame, int32_t* o_label,
                          int64_t* o_count, int64_t* o_first, float* o_cx, float* o_cy,
                          float* o_mi, int64_t* frame_first_noise, int64_t* n_seg_host,
                          hipStream_t st) {
  if (n < 0 || n_frames < 0 || n_clusters < 0 || !n_seg_host) {
    set_error("rpt_cluster_summaries: bad arguments");
    return RPT_EINVAL;
  }
  // the summarize grid is sized for one wave per run component once the count is known; a
  // frame with more than kFsMaxKeys labels sends K9 to the radix path
  const int32_t* nd = nullptr;
  int32_t n_seg = 0;
  for (int pass = 0; pass < 2; ++pass) {
    RPT_TRY(summaries_impl(labels, x, y, inten, FramesPf{pf}, n, n_frames,
                           radix_bits_for(n_clusters),
                           (int64_t)n_clusters * std::max(n_frames, 1) + 1, o_frame, o_label,
                           o_count, o_first, o_cx, o_cy, o_mi, frame_first_noise, &nd, pass == 1,
                           nullptr, st));
    RPT_HIP(hipMemcpyAsync(&n_seg, nd, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RPT_TRY(wait_stream(st));
    if (n_seg >= 0) break;
  }
  *n_seg_host = n_seg;
  return RPT_OK;
}

int32_t cluster_summaries_dev(const int32_t* labels, const float* x, const float* y,
                              const float* inten, const int32_t* pf, int64_t n, int32_t n_frames,
                              int bits, int64_t s_hint, int32_t* o_frame, int32_t* o_label,
                              int64_t* o_count, int64_t* o_first, float* o_cx, float* o_cy,
                              float* o_mi, int64_t* frame_first_noise,
                              const int32_t** n_seg_dev, bool force_radix, bool* radix_used,
                              hipStream_t st, const int64_t* frame_off,
                              const uint8_t* inten8) {
  if (n < 0 || n_frames < 0 || bits < 1 || bits > 32 || !n_seg_dev ||
      (frame_off != nullptr) != (inten8 != nullptr)) {
    set_error("cluster_summaries_dev: bad arguments");
    return RPT_EINVAL;
  }
  auto run = [&](auto inten_, auto fr) {
    return summaries_impl(labels, x, y, inten_, fr, n, n_frames, bits, s_hint, o_frame, o_label,
                          o_count, o_first, o_cx, o_cy, o_mi, frame_first_noise, n_seg_dev,
                          force_radix, radix_used, st);
  };
  return frame_off ? run(inten8, FramesOff{frame_off, n_frames}) : run(inten, FramesPf{pf});
}

int32_t label_means(const int32_t* labels, const float* x, const float* y, const float* inten,
                    int64_t n, int64_t n_labels, int64_t* o_count, float* o_x, float* o_y,
                    float* o_v, hipStream_t st) {
  if (n < 0 || n_labels < 0 || (n > 0 && (!labels || !x || !y || !inten)) ||
      (n_labels > 0 && (!o_count || !o_x || !o_y || !o_v))) {
    set_error("rpt_label_means: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31) - 1 || n_labels >= (int64_t(1) << 31) - 1) {
    set_error("rpt_label_means: n exceeds the int32 index space");
    return RPT_ENOTSUP;
  }
  if (n_labels > 0) {
    RPT_HIP(hipMemsetAsync(o_count, 0, sizeof(int64_t) * (size_t)n_labels, st));
    RPT_HIP(hipMemsetAsync(o_x, 0, sizeof(float) * (size_t)n_labels, st));
    RPT_HIP(hipMemsetAsync(o_y, 0, sizeof(float) * (size_t)n_labels, st));
    RPT_HIP(hipMemsetAsync(o_v, 0, sizeof(float) * (size_t)n_labels, st));
  }
  if (n == 0) return wait_stream(st);
  RadixFront<float> r;
  RPT_TRY(radix_front(
      scratch(st), labels, x, y, inten, n, radix_bits_for(n_labels + 1),
      [&](int g, const uint32_t* sk, const uint32_t*, int32_t* head) {
        hipLaunchKernelGGL(k_label_heads, dim3(g), dim3(kBlock), 0, st, sk, n, head);
      },
      st, &r));
  hipLaunchKernelGGL(k_label_means, dim3(grid_for(3 * (n_labels + 1), kBlock / 64, 16384)),
                     dim3(kBlock), 0, st, r.sk, r.seg_start, r.pos + n, n, r.gx, r.gy, r.gi,
                     n_labels, o_count, o_x, o_y, o_v);
  RPT_CHECK_LAUNCH();
  return wait_stream(st);
}

}  // namespace rpt
