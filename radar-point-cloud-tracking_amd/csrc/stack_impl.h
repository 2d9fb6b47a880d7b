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
// The land grid's edges over b4 = {min x, max x, min y, max y}: arange_edges per axis.
struct LandEdges {
  std::vector<double> xe, ye;
  int32_t nxe() const { return (int32_t)xe.size(); }
  int32_t nye() const { return (int32_t)ye.size(); }
  int64_t cells() const {  // 0: degenerate
    return nxe() < 2 || nye() < 2 ? 0 : (int64_t)(nxe() - 1) * (nye() - 1);
  }
};
inline LandEdges land_edges(const float* b4, double res) {
  return LandEdges{arange_edges(b4[0], b4[1], res), arange_edges(b4[2], b4[3], res)};
}

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
// The packed readback of the stack driver's K9 results, capacity sc segments over F frames:
//   [S, n_clusters or -1] [count sc] [first sc] [first noise F] [frame sc] [label sc]
//   [cx sc] [cy sc] [mi sc]
// k_pack_segs writes it on the device and rpt_stack::read_segs decodes it on the host.
struct SegPackOut {
  int64_t *hdr, *count, *first, *noise;
  int32_t *frame, *label;
  float *cx, *cy, *mi;
  __host__ __device__ SegPackOut(char* base, int64_t sc, int32_t F) {
    hdr = reinterpret_cast<int64_t*>(base);
    count = hdr + 2;
    first = count + sc;
    noise = first + sc;
    frame = reinterpret_cast<int32_t*>(noise + F);
    label = frame + sc;
    cx = reinterpret_cast<float*>(label + sc);
    cy = cx + sc;
    mi = cy + sc;
  }
};
inline size_t seg_pack_bytes(int64_t sc, int32_t F) {  // (the end of mi)
  return 16 + (size_t)sc * (8 + 8 + 4 + 4 + 4 + 4 + 4) + (size_t)F * 8;
}

// Grow-only buffers that own their memory.  Neither may live in an object of static storage
// duration: the HIP runtime may be gone before a static destructor frees.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
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
};

struct PinnedBuf {
  char* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
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
  // ev[t % kRing]: recorded after ticket t's K1; all created by rpt_k1_gate_create
  hipEvent_t ev[kRing] = {};
  ~rpt_k1_gate() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// What one stage of rpt_stack::run leaves for the next.
struct rpt_stack_stage {
  float *cx = nullptr, *cy = nullptr, *cv = nullptr;  // the current points: cv and cpf in the
  uint8_t* cv8 = nullptr;                             // wide layout, cv8 in the narrow one
  int32_t* cpf = nullptr;
  int64_t n_in = 0;
  bool k1_bounds = false;            // the K1 write left the points' xy bounds in k1_bnd
  const int64_t* fo_k9 = nullptr;    // narrow: device frame offsets of the points K4-K9 see
  const int32_t* ncl_dev = nullptr;  // ST-DBSCAN's cluster count, still on the device
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

  ~rpt_stack() {  // (the buffers free themselves)
    if (ev_ok)
      for (auto& e : ev) (void)hipEventDestroy(e);
    if (ev_rb) (void)hipEventDestroy(ev_rb);
  }

  // ---- what the stack driver and the shard driver both do
  // fo_k1 = the frame offsets from the read-back file offsets (F frames x G files); returns the
  // number of frames that hold a K1 point
  int32_t set_fo_k1(const int64_t* hfo, int32_t F, int32_t G) {
    fo_k1.resize((size_t)F + 1);
    for (int32_t f = 0; f <= F; ++f) fo_k1[(size_t)f] = hfo[(size_t)f * G];
    int32_t n_built = 0;
    for (int32_t f = 0; f < F; ++f) n_built += (fo_k1[(size_t)f + 1] > fo_k1[(size_t)f]) ? 1 : 0;
    return n_built;
  }
  // e into edges as [x edges | y edges | tail (n_tail int64, optional)], staged in up: ONE
  // upload; *tail_dev (nullable) = where the tail landed on the device  (stack.cpp)
  int32_t upload_land_edges(const rpt::LandEdges& e, const int64_t* tail, size_t n_tail,
                            hipStream_t st, const int64_t** tail_dev);
  // K9's outputs for up to cap2 segments over F frames, and their pointers for a pack kernel
  int32_t ensure_segs(size_t cap2, int32_t F, hipStream_t st) {
    RPT_TRY(seg_frame.ensure(cap2, st));
    RPT_TRY(seg_label.ensure(cap2, st));
    RPT_TRY(seg_count.ensure(cap2, st));
    RPT_TRY(seg_first.ensure(cap2, st));
    RPT_TRY(seg_cx.ensure(cap2, st));
    RPT_TRY(seg_cy.ensure(cap2, st));
    RPT_TRY(seg_mi.ensure(cap2, st));
    return first_noise.ensure((size_t)std::max(F, 1), st);
  }
  rpt::SegPack seg_pack() const {
    return rpt::SegPack{seg_count.p, seg_first.p, first_noise.p, seg_frame.p,
                        seg_label.p, seg_cx.p,    seg_cy.p,      seg_mi.p};
  }

  bool had_gain = false;  // the last run wrote per-point gains (gain table given)
  void* db_state = nullptr;      // the last run's ST-DBSCAN state (per device and stream) ...
  hipStream_t db_stream = nullptr;  // ... and its stream (rpt_stack_core_flags)
  int32_t run(const rpt_stack_params& p, const void* echo, const float* scale,
              const float* cos_t, const float* sin_t, const int32_t* gain, rpt_stack_result* out,
              hipStream_t st);

 private:  // run's stages, in order (stack.cpp); s: what each leaves for the next
  int32_t run_k1(const rpt_stack_params& p, const void* echo, const float* scale,
                 const float* cos_t, const float* sin_t, const int32_t* gain, hipStream_t st,
                 rpt_stack_stage& s, rpt_stack_result& r);
  int32_t run_land(const rpt_stack_params& p, const int32_t* gain, hipStream_t st,
                   rpt_stack_stage& s, rpt_stack_result& r);
  int32_t run_stdbscan(const rpt_stack_params& p, hipStream_t st, rpt_stack_stage& s,
                       rpt_stack_result& r);
  int32_t run_k9(const rpt_stack_params& p, hipStream_t st, const rpt_stack_stage& s,
                 rpt_stack_result& r);
  int32_t read_segs(const int32_t* nseg_dev, const int32_t* ncl_dev, int64_t sc, hipEvent_t mark,
                    hipStream_t st, int64_t* S);
};

