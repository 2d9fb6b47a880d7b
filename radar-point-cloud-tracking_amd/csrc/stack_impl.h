// Internals shared by the native stack driver (stack.cpp) and the frame-sharded driver
// (shard.cpp): grow-only device / pinned buffers, the library stages they call, and the stack
// handle (whose K1 / land / K9 buffers the shard handle reuses).
#pragma once
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "dist.h"       // the shard merge's device steps
#include "land.h"       // bounds, K2 / K3
#include "polar.h"      // K1 and the small kernels beside it
#include "stdbscan.h"   // K4-K8, fused and phased
#include "summaries.h"  // K9, radix_bits_for

namespace rpt {

std::vector<double> arange_edges(float lo, float hi, double res);

struct SegPack {
  const int64_t* count;
  const int64_t* first;
  const int64_t* noise;
  const int32_t* frame;
  const int32_t* label;
  const float* cx;
  const float* cy;
  const float* mi;
};
inline size_t seg_pack_bytes(int64_t sc, int32_t F) {
  return 16 + (size_t)sc * (8 + 8 + 4 + 4 + 4 + 4 + 4) + (size_t)F * 8;
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  // grows only between syncs of the owning stream (callers synchronise before growing)
  int32_t ensure(size_t n, hipStream_t st) {
    if (n <= cap && p) return RPT_OK;
    if (p) {
      RPT_HIP(hipStreamSynchronize(st));
      RPT_HIP(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    const size_t want = std::max<size_t>(n + n / 8 + 64, 256);
    if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) {
      p = nullptr;
      set_error("rpt_stack: hipMalloc of %zu bytes failed", want * sizeof(T));
      return RPT_ENOMEM;
    }
    cap = want;
    return RPT_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct PinnedBuf {
  char* p = nullptr;
  size_t cap = 0;
  int32_t ensure(size_t bytes, hipStream_t st) {
    if (bytes <= cap && p) return RPT_OK;
    if (p) {
      RPT_HIP(hipStreamSynchronize(st));
      RPT_HIP(hipHostFree(p));
      p = nullptr;
      cap = 0;
    }
    const size_t want = align_up(bytes + bytes / 8 + 4096, 4096);
    if (hipHostMalloc((void**)&p, want, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      set_error("rpt_stack: hipHostMalloc of %zu bytes failed", want);
      return RPT_ENOMEM;
    }
    cap = want;
    return RPT_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};


}  // namespace rpt

using rpt::DevBuf;
using rpt::PinnedBuf;
// K1 turns of several stack handles (lanes): each run's K1 (count + write, HBM-bound) is
// enqueued only after the previous run's, and its stream waits on the device for that one to end,
// so the lanes' K1 passes never share the HBM and always overlap other lanes' latency-bound
// stages.  Turns go in arrival order (a run takes the next ticket when it reaches K1): a waiting
// run only waits for runs already inside their K1 enqueue, so no cycle can form.
struct rpt_k1_gate {
  static constexpr int kRing = 16;
  std::mutex mu;
  std::condition_variable cv;
  int64_t issued = 0, next = 0;  // tickets handed out / the ticket whose turn it is
  hipEvent_t ev[kRing] = {};     // ev[t % kRing]: recorded after ticket t's K1
  ~rpt_k1_gate() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct rpt_stack {
  DevBuf<uint32_t> pack_d;  // packed readback staging
  rpt_k1_gate* k1_gate = nullptr;  // (not owned) rpt_stack_set_k1_gate
  DevBuf<int64_t> row_prefix, file_off, new_off, first_noise, seg_count, seg_first, scal;
  DevBuf<int64_t> fo_d;  // narrow path without the land filter: the K1 frame offsets
  DevBuf<uint16_t> land_cell16;  // narrow path: the land cells of a grid of <= 65,536 cells
  DevBuf<uint8_t> v8, v8b;       // narrow path: the intensities (u8 samples), K1's and the kept
  bool narrow = false;   // the last run kept no per-point frame slots (pf, pf2 unused)
  DevBuf<float> x, y, v, x2, y2, v2, t, seg_cx, seg_cy, seg_mi;
  DevBuf<int32_t> g, pf, g2, pf2, labels, land_cnt, land_cell, seg_frame, seg_label;
  DevBuf<double> land_tot, edges;
  DevBuf<uint8_t> land_mask;
  DevBuf<uint32_t> k1_stage;           // K1 staged kept samples (count pass -> write pass)
  DevBuf<uint32_t> k1_bnd;             // K1 write's xy bounds + block partials
  DevBuf<uint8_t> bnd;                 // ST-DBSCAN bounds (+ partials) of the kept points
  std::vector<char> dbscan_bounds;     // their host copy, from the land readback
  PinnedBuf up, down;  // host staging: uploads (edges, offsets), readbacks
  std::vector<int64_t> fo_k1, fo_in;
  std::vector<int32_t> h_frame, h_label;
  std::vector<int64_t> h_count, h_first, h_noise;
  std::vector<float> h_cx, h_cy, h_mi;
  bool land_applied = false;
  int32_t n_frames = 0;
  int64_t n_in = 0;
  hipEvent_t ev[5] = {};
  bool ev_ok = false;
  hipEvent_t ev_rb = nullptr;  // readback marker of the speculative K1 write
  int sum_bits = 12;           // radix bits of the K9 label keys, from the previous run
  bool k9_radix = false;       // a frame held more labels than K9's frame sort takes
  int64_t seg_hint = 0;        // segment-count estimate from the previous run

  ~rpt_stack() {
    DevBuf<int64_t>* i64[] = {&row_prefix, &file_off, &new_off, &first_noise, &seg_count,
                              &seg_first, &scal};
    for (auto* b : i64) b->release();
    fo_d.release();
    land_cell16.release();
    v8.release();
    v8b.release();
    DevBuf<float>* f32[] = {&x, &y, &v, &x2, &y2, &v2, &t, &seg_cx, &seg_cy, &seg_mi};
    for (auto* b : f32) b->release();
    DevBuf<int32_t>* i32[] = {&g,        &pf,       &g2,        &pf2,      &labels,
                              &land_cnt, &land_cell, &seg_frame, &seg_label};
    for (auto* b : i32) b->release();
    land_tot.release();
    edges.release();
    pack_d.release();
    bnd.release();
    land_mask.release();
    k1_stage.release();
    k1_bnd.release();
    up.release();
    down.release();
    if (ev_ok)
      for (auto& e : ev) (void)hipEventDestroy(e);
    if (ev_rb) (void)hipEventDestroy(ev_rb);
  }

  bool had_gain = false;  // the last run wrote per-point gains (gain table given)
  void* db_state = nullptr;      // the last run's ST-DBSCAN state (per device and stream) ...
  hipStream_t db_stream = nullptr;  // ... and its stream (rpt_stack_core_flags)
  int32_t run(const rpt_stack_params& p, const void* echo, const float* scale,
              const float* cos_t, const float* sin_t, const int32_t* gain, rpt_stack_result* out,
              hipStream_t st);
};

