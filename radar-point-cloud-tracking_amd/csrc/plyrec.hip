// Binary PLY records of the denoise pipeline's writer on the device (write_ply,
// PointCloudWorkF/stdbscan_denoising_pipeline.py:767-855): the [signal_mask] indexing, the tab20 /
// viridis colours and the 15-byte structured-array records in one pass over the points.  The
// per-value rules are plyrec.h's, shared with the host (plyrec.cpp).
//
// Two passes around the library's scan, over tiles of plyrec::kTile = 1024 points:
//   k_ply_count   kept points per tile and the largest label -> exclusive scan -> tile offsets
//   k_ply_write   one block of 256 threads per tile, four rounds of 256 points.  A wave ranks its
//                 kept points by ballot and popcount; the 16 wave counts of the tile, summed in
//                 order, give every wave-round its prefix.  A kept point's record is staged in LDS
//                 at 15 * (its rank in the tile) behind the 16-byte phase of the tile's first
//                 byte in out, so the staged image and the tile's byte range in global memory
//                 are aligned alike.  A record starts at any byte residue: its four words are
//                 shifted to that residue and stored as whole words where the record fills
//                 them and as 1- and 2-byte pieces at its two ends (neighbours share the word at
//                 their seam, never a byte: plain LDS stores, nothing to zero).  The block then
//                 copies the image out: 16-byte vector stores for the aligned interior, single
//                 byte stores for the ragged head and tail.
//
// Neighbouring tiles never write the same byte but may share a 16-byte (or 4-byte) word, and
// their blocks run concurrently: the interior stores cover only words that lie wholly inside the
// tile's own range, and the head and tail bytes go out one by one -- no word is read-modified.
// The kernel reads 12-16 bytes and writes 15 bytes a kept point.
#include "common.h"
#include "plyrec.h"

namespace rpt {
namespace {
namespace pr = plyrec;

constexpr int kBlock = 256;
constexpr int kRounds = pr::kTile / kBlock;
constexpr int kWaves = kBlock / kWave;
constexpr int kSlots = kRounds * kWaves;  // wave-rounds of a tile, in point order
// the records behind the 16-byte phase of the tile's first byte
constexpr int kStageBytes = pr::kTile * pr::kRecord + 16;
static_assert(kStageBytes % 16 == 0, "the image is copied out in 16-byte pieces");

// The 15 bytes of the record w (plyrec::words) at byte b of the image, b of any residue: q is the
// word that holds byte b, the record's byte j is q's byte s + j.  Shifted by s bytes the record
// covers the words 1 and 2 wholly, word 3 wholly unless s == 0, and pieces of the words 0 and 4.
__device__ __forceinline__ void stage_record(uint32_t* stage, int b, const uint32_t w[4]) {
  const int s = b & 3, sh = 32 - 8 * s;
  uint32_t* q = stage + (b >> 2);
  uint8_t* q8 = reinterpret_cast<uint8_t*>(q);
  uint16_t* q16 = reinterpret_cast<uint16_t*>(q);
  const uint32_t v0 = w[0] << (8 * s);
  const uint32_t v3 = (uint32_t)((((uint64_t)w[3] << 32) | w[2]) >> sh);
  const uint32_t v4 = (uint32_t)((uint64_t)w[3] >> sh);  // (sh == 32 for s == 0: zero, unused)
  q[1] = (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> sh);
  q[2] = (uint32_t)((((uint64_t)w[2] << 32) | w[1]) >> sh);
  switch (s) {
    case 0:  // bytes 0..3 | 12, 13 | 14
      q[0] = v0;
      q16[6] = (uint16_t)v3;
      q8[14] = (uint8_t)(v3 >> 16);
      break;
    case 1:  // byte 1 | 2, 3 | 12..15
      q8[1] = (uint8_t)(v0 >> 8);
      q16[1] = (uint16_t)(v0 >> 16);
      q[3] = v3;
      break;
    case 2:  // bytes 2, 3 | 12..15 | 16
      q16[1] = (uint16_t)(v0 >> 16);
      q[3] = v3;
      q8[16] = (uint8_t)v4;
      break;
    default:  // byte 3 | 12..15 | 16, 17
      q8[3] = (uint8_t)(v0 >> 24);
      q[3] = v3;
      q16[8] = (uint16_t)v4;
      break;
  }
}
constexpr int kColorBlock = 256;

__global__ void __launch_bounds__(kBlock)
k_ply_count(const int32_t* __restrict__ labels, int64_t n, int signal_only,
            int32_t* __restrict__ counts, uint32_t* __restrict__ max_plus1) {
  __shared__ uint32_t sh_cnt, sh_max;
  if (threadIdx.x == 0) {
    sh_cnt = 0;
    sh_max = 0;
  }
  __syncthreads();
  const int64_t first = (int64_t)blockIdx.x * pr::kTile;
  const bool has_labels = labels != nullptr;
  uint32_t c = 0, m = 0;
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    const int64_t i = first + k * kBlock + threadIdx.x;
    if (i < n) {
      const int32_t lab = has_labels ? labels[i] : 0;
      c += pr::keep(has_labels, signal_only != 0, lab);
      if (has_labels && lab >= 0) m = max(m, (uint32_t)lab + 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c += (uint32_t)__shfl_xor((int)c, off);
    m = max(m, (uint32_t)__shfl_xor((int)m, off));
  }
  if (lane_id() == 0) {
    atomicAdd(&sh_cnt, c);
    atomicMax(&sh_max, m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = (int32_t)sh_cnt;
    if (sh_max) atomicMax(max_plus1, sh_max);
  }
}

__global__ void __launch_bounds__(kBlock)
k_ply_write(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
            const int32_t* __restrict__ labels, int signal_only, const uint8_t* __restrict__ lut,
            int64_t n, const int64_t* __restrict__ off, uint8_t* __restrict__ out,
            int64_t out_bytes) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[kStageBytes / 4];
  __shared__ int cnt[kSlots];
  const int tid = (int)threadIdx.x;
  const int wave = tid / kWave;
  const int64_t first = (int64_t)blockIdx.x * pr::kTile;
  const int64_t o0 = off[blockIdx.x], o1 = off[blockIdx.x + 1];
  // offsets that are not this input's (or an out too small): the block writes nothing
  if (o0 < 0 || o1 < o0 || o1 - o0 > pr::kTile || o1 > out_bytes / pr::kRecord) return;
  const bool has_labels = labels != nullptr;
  uint32_t w[kRounds][4];
  int rank[kRounds];
  bool kp[kRounds];
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    const int64_t i = first + k * kBlock + tid;
    const int32_t lab = (i < n && has_labels) ? labels[i] : 0;
    kp[k] = i < n && pr::keep(has_labels, signal_only != 0, lab);
    const uint64_t mask = __ballot(kp[k]);
    rank[k] = rank_in_mask(mask);
    if (lane_id() == 0) cnt[k * kWaves + wave] = __popcll(mask);
    if (kp[k]) {
      const float zi = z[i];
      pr::words(x[i], y[i], zi, pr::color(lut, has_labels, lab, zi), w[k]);
    }
  }
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(out) + (uintptr_t)(o0 * pr::kRecord);
  const int lo = (int)(a0 & 15u);  // byte k of the image is the byte at (a0 - lo) + k
  const int hi = lo + (int)(o1 - o0) * pr::kRecord;
  __syncthreads();  // cnt
  int total = 0;
  int pre[kRounds] = {};
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int c = cnt[j];
    total += c;
#pragma unroll
    for (int k = 0; k < kRounds; ++k)
      if (j < k * kWaves + wave) pre[k] += c;
  }
  // the tile's own kept count against its offsets (the same for every thread of the block):
  // with it every byte of [lo, hi) is staged by exactly one record
  if (total != (int)(o1 - o0)) return;
#pragma unroll
  for (int k = 0; k < kRounds; ++k)
    if (kp[k]) stage_record(stage, lo + (pre[k] + rank[k]) * pr::kRecord, w[k]);  // ends <= hi
  __syncthreads();
  const uint8_t* img = reinterpret_cast<const uint8_t*>(stage);
  uint8_t* base = reinterpret_cast<uint8_t*>(a0 - (uintptr_t)lo);  // 16-byte aligned
  const int vlo = (lo + 15) & ~15, vhi = hi & ~15;
  const int head_end = min(vlo, hi);
  for (int k = lo + tid; k < head_end; k += kBlock) base[k] = img[k];
  for (int k = vlo + 16 * tid; k < vhi; k += 16 * kBlock)
    *reinterpret_cast<uint4*>(base + k) = *reinterpret_cast<const uint4*>(img + k);
  for (int k = max(vhi, vlo) + tid; k < hi; k += kBlock) base[k] = img[k];
}

__global__ void __launch_bounds__(kColorBlock)
k_ply_colors(const float* __restrict__ z, const int32_t* __restrict__ labels,
             const uint8_t* __restrict__ lut, int64_t n, uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * kColorBlock + threadIdx.x;
  if (i >= n) return;
  const bool has_labels = labels != nullptr;
  const uint32_t c = pr::color(lut, has_labels, has_labels ? labels[i] : 0,
                               has_labels ? 0.0f : z[i]);
  rgb[3 * i] = (uint8_t)c;
  rgb[3 * i + 1] = (uint8_t)(c >> 8);
  rgb[3 * i + 2] = (uint8_t)(c >> 16);
}
}  // namespace
}  // namespace rpt

extern "C" int32_t rpt_ply_records_size(const int32_t* labels, int64_t n, int32_t signal_only,
                                        int64_t* tile_offsets, int64_t* n_kept_host,
                                        int32_t* max_label_host, void* stream) {
  rpt::clear_error();
  if (n < 0 || !tile_offsets || !n_kept_host || (signal_only && !labels)) {
    rpt::set_error("rpt_ply_records_size: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31)) {
    rpt::set_error("rpt_ply_records_size: n=%lld exceeds the int32 index space", (long long)n);
    return RPT_ENOTSUP;
  }
  *n_kept_host = 0;
  if (max_label_host) *max_label_host = -1;
  hipStream_t st = rpt::as_stream(stream);
  if (n == 0) {
    RPT_HIP(hipMemsetAsync(tile_offsets, 0, sizeof(int64_t), st));
    return rpt::wait_stream(st);
  }
  const int64_t tiles = rpt_ply_record_tiles(n);
  rpt::Scratch& sc = rpt::scratch(st);
  rpt::Budget bud;
  bud.add<int32_t>((size_t)tiles);
  RPT_TRY(sc.reserve(bud.bytes, st));
  int32_t* counts = sc.carve_n<int32_t>((size_t)tiles);
  uint32_t* max_plus1 = nullptr;
  RPT_TRY(rpt::zero_n(st, 1, &max_plus1));
  hipLaunchKernelGGL(rpt::k_ply_count, dim3((unsigned)tiles), dim3(rpt::kBlock), 0, st, labels, n,
                     (int)(signal_only != 0), counts, max_plus1);
  RPT_CHECK_LAUNCH();
  RPT_TRY(rpt::exclusive_scan_total_i32_to_i64(counts, tile_offsets, tiles, st));
  int64_t kept = 0;
  uint32_t mx = 0;
  RPT_HIP(hipMemcpyAsync(&kept, tile_offsets + tiles, sizeof(kept), hipMemcpyDeviceToHost, st));
  RPT_HIP(hipMemcpyAsync(&mx, max_plus1, sizeof(mx), hipMemcpyDeviceToHost, st));
  RPT_TRY(rpt::wait_stream(st));
  *n_kept_host = kept;
  if (max_label_host) *max_label_host = (int32_t)((int64_t)mx - 1);
  return RPT_OK;
}

extern "C" int32_t rpt_ply_records_write(const float* x, const float* y, const float* z,
                                         const int32_t* labels, int32_t signal_only,
                                         const uint8_t* lut, int64_t n,
                                         const int64_t* tile_offsets, uint8_t* out,
                                         int64_t out_bytes, void* stream) {
  rpt::clear_error();
  if (n < 0 || out_bytes < 0 || (signal_only && !labels) ||
      (n > 0 && (!x || !y || !z || !lut || !tile_offsets || (out_bytes > 0 && !out)))) {
    rpt::set_error("rpt_ply_records_write: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31)) {
    rpt::set_error("rpt_ply_records_write: n=%lld exceeds the int32 index space", (long long)n);
    return RPT_ENOTSUP;
  }
  if (n == 0) return RPT_OK;
  hipStream_t st = rpt::as_stream(stream);
  hipLaunchKernelGGL(rpt::k_ply_write, dim3((unsigned)rpt_ply_record_tiles(n)),
                     dim3(rpt::kBlock), 0, st, x, y, z, labels, (int)(signal_only != 0), lut, n,
                     tile_offsets, out, out_bytes);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}

extern "C" int32_t rpt_ply_colors(const float* z, const int32_t* labels, const uint8_t* lut,
                                  int64_t n, uint8_t* rgb, void* stream) {
  rpt::clear_error();
  if (n < 0 || (n > 0 && ((!z && !labels) || !lut || !rgb))) {
    rpt::set_error("rpt_ply_colors: bad arguments");
    return RPT_EINVAL;
  }
  if (n >= (int64_t(1) << 31)) {
    rpt::set_error("rpt_ply_colors: n=%lld exceeds the int32 index space", (long long)n);
    return RPT_ENOTSUP;
  }
  if (n == 0) return RPT_OK;
  hipStream_t st = rpt::as_stream(stream);
  const dim3 grid((unsigned)((n + rpt::kColorBlock - 1) / rpt::kColorBlock));
  hipLaunchKernelGGL(rpt::k_ply_colors, grid, dim3(rpt::kColorBlock), 0, st, z, labels, lut, n,
                     rgb);
  RPT_CHECK_LAUNCH();
  return RPT_OK;
}
