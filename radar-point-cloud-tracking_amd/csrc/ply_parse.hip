// ASCII rows of decimal numbers -> float32 columns on the device: the vertex lines of load_ply
// (radar_pipeline/core/loaders.py:149-220, one float() per token), the reverse of text.hip.
//
// Three passes around the library's scan.  The text is cut into tiles of kTileBytes; a block of
// 256 threads takes one tile, each wave a contiguous quarter of it, each lane 16 bytes per load.
//   k_count   '\n' per tile, and the count of bytes outside "0-9 + - . space tab \r \n" and of
//             '\r' not followed by '\n' (the next byte may lie in the next tile)
//   scan      exclusive prefix of the tile counts
//   k_starts  row_start[j] = byte offset of line j for j <= n_rows: a '\n' of rank r in the text
//             ends line r and starts line r + 1.  Rank in the tile: a wave prefix over the lanes'
//             counts per load, the loads of a wave in order, the waves through LDS.
//   k_parse   a wave takes 64 consecutive rows, stages their byte span in LDS by 16-byte loads
//             and every lane splits its own row at blanks and parses the tokens (parse32.h) into
//             out[c * n_rows + i]: column-major, a column store of a wave is contiguous.  A wave
//             whose span exceeds its LDS share reads global memory per lane instead.
// A row with another token count than n_cols, a token outside parse32's domain or more than
// kRowMaxBytes bytes is counted; the caller then discards the output and reads on the host.
//
// Memory safety does not depend on the bytes: every load is guarded by nbytes (16-byte loads only
// where all 16 bytes are inside and the base is 16-byte aligned, byte loads otherwise), row
// offsets are checked against each other and nbytes before use, and a store needs c < n_cols and
// i < n_rows (row_start: index <= n_rows).
#include "common.h"
#include "parse32.h"
#include "text.h"

namespace rpt {
namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kLoadsPerLane = 4;
constexpr int kWaveBytes = kWave * 16 * kLoadsPerLane;  // 4096: a wave's part of a tile
constexpr int kTileBytes = kWaves * kWaveBytes;         // 16384
constexpr int kStageBytes = 6144;                       // LDS of one wave's 64 rows (96 a row)
constexpr int kRowMaxBytes = kStageBytes - 16;  // fits behind any 16-byte phase of its start

// bit b: byte b may occur in a body ("0-9 + - . space tab \r \n"; all below 64)
constexpr uint64_t kAllowed = (0x3ffull << '0') | (1ull << '+') | (1ull << '-') | (1ull << '.') |
                              (1ull << ' ') | (1ull << '\t') | (1ull << '\r') | (1ull << '\n');

struct Bytes16 {
  uint8_t b[16];
};

// text[off .. off + 16) with ' ' for the bytes at and past nbytes; off >= 0.
__device__ __forceinline__ Bytes16 load16(const uint8_t* __restrict__ text, int64_t nbytes,
                                          int64_t off, bool aligned) {
  Bytes16 r;
  if (aligned && off + 16 <= nbytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + off);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) r.b[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) r.b[k] = off + k < nbytes ? text[off + k] : (uint8_t)' ';
  }
  return r;
}

__device__ __forceinline__ uint32_t newline_mask(const Bytes16& v) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) m |= (uint32_t)(v.b[k] == '\n') << k;
  return m;
}

// offset in the text of the 16 bytes lane `lane` of wave `wave` reads in load j of tile `tile`
__device__ __forceinline__ int64_t chunk_offset(int64_t tile, int wave, int j, int lane) {
  return tile * kTileBytes + wave * kWaveBytes + j * (kWave * 16) + lane * 16;
}

__global__ void __launch_bounds__(kBlock)
k_count(const uint8_t* __restrict__ text, int64_t nbytes, int32_t* __restrict__ tile_lines,
        unsigned long long* __restrict__ n_bad) {
  __shared__ int s_lines[kWaves];
  const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
  const int wave = threadIdx.x / kWave, lane = lane_id();
  int lines = 0, bad = 0;
#pragma unroll
  for (int j = 0; j < kLoadsPerLane; ++j) {
    const int64_t off = chunk_offset(blockIdx.x, wave, j, lane);
    if (off >= nbytes) break;
    const Bytes16 v = load16(text, nbytes, off, aligned);
    lines += __popc(newline_mask(v));
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t c = v.b[k];
      bad += !(c < 64u && ((kAllowed >> c) & 1ull));
      if (c == '\r') {
        uint32_t next;
        if (k < 15)
          next = off + k + 1 < nbytes ? v.b[k + 1] : 0u;
        else
          next = off + 16 < nbytes ? text[off + 16] : 0u;
        bad += next != '\n';
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lines += __shfl_xor(lines, d);
    bad += __shfl_xor(bad, d);
  }
  if (lane == 0) {
    s_lines[wave] = lines;
    if (bad) atomicAdd(n_bad, (unsigned long long)bad);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kWaves; ++w) t += s_lines[w];
    tile_lines[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kBlock)
k_starts(const uint8_t* __restrict__ text, int64_t nbytes, const int64_t* __restrict__ tile_base,
         int64_t n_tiles, int64_t n_rows, uint32_t* __restrict__ row_start) {
  __shared__ int s_lines[kWaves];
  const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
  const int wave = threadIdx.x / kWave, lane = lane_id();
  const int64_t base = tile_base[blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    row_start[0] = 0u;
    // fewer '\n' than rows: the last row may end at the end of the text
    if (tile_base[n_tiles] < n_rows) row_start[n_rows] = (uint32_t)nbytes;
  }
  if (base >= n_rows) return;  // every line that starts behind this tile's '\n' is past n_rows
  uint32_t mask[kLoadsPerLane];
  int before[kLoadsPerLane];  // '\n' of this wave in front of the lane's bytes of load j
  int wave_lines = 0;
#pragma unroll
  for (int j = 0; j < kLoadsPerLane; ++j) {
    const int64_t off = chunk_offset(blockIdx.x, wave, j, lane);
    mask[j] = off < nbytes ? newline_mask(load16(text, nbytes, off, aligned)) : 0u;
    const int c = __popc(mask[j]);
    int incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    before[j] = wave_lines + incl - c;
    wave_lines += __shfl(incl, kWave - 1);
  }
  if (lane == 0) s_lines[wave] = wave_lines;
  __syncthreads();
  int64_t rank0 = base;
  for (int w = 0; w < wave; ++w) rank0 += s_lines[w];
#pragma unroll
  for (int j = 0; j < kLoadsPerLane; ++j) {
    const int64_t off = chunk_offset(blockIdx.x, wave, j, lane);
    int64_t r = rank0 + before[j];
    uint32_t m = mask[j];
    while (m) {
      const int k = __ffs(m) - 1;
      m &= m - 1u;
      ++r;  // the '\n' of rank r - 1 starts line r
      if (r <= n_rows) row_start[r] = (uint32_t)(off + k + 1);
    }
  }
}

__device__ __forceinline__ bool blank(uint32_t c) { return c == ' ' || c == '\t'; }

// One row p[0..len) (line end included): its tokens into out[c * n_rows + i].  false: the row is
// outside the domain (the values stored for it are then meaningless, but inside out).
__device__ __forceinline__ bool parse_row(const uint8_t* p, int len, int n_cols, int64_t n_rows,
                                          int64_t i, float* __restrict__ out) {
  if (len > 0 && p[len - 1] == '\n') --len;
  if (len > 0 && p[len - 1] == '\r') --len;
  int c = 0;
  bool ok = true;
  int k = 0;
  while (k < len) {
    if (blank(p[k])) {
      ++k;
      continue;
    }
    int e = k + 1;
    while (e < len && !blank(p[e])) ++e;
    float v;
    if (c < n_cols && parse32::parse(p + k, e - k, &v))
      out[(int64_t)c * n_rows + i] = v;
    else
      ok = false;
    ++c;
    k = e;
  }
  return ok && c == n_cols;
}

__global__ void __launch_bounds__(kBlock)
k_parse(const uint8_t* __restrict__ text, int64_t nbytes, const uint32_t* __restrict__ row_start,
        int64_t n_rows, int n_cols, float* __restrict__ out,
        unsigned long long* __restrict__ n_bad) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[kWaves][kStageBytes];
  const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
  const int wave = threadIdx.x / kWave, lane = lane_id();
  const int64_t r0 = ((int64_t)blockIdx.x * kWaves + wave) * kWave;
  const int64_t r1 = min(r0 + kWave, n_rows);
  uint8_t* stage = s_stage[wave];
  int64_t lo = 0, hi = 0, a = 0;
  bool staged = false;
  if (r0 < n_rows) {
    lo = row_start[r0];
    hi = row_start[r1];
    a = lo & ~(int64_t)15;
    staged = lo <= hi && hi <= nbytes && hi - a <= kStageBytes;
    if (staged) {
      for (int64_t o = lane * 16; o < hi - a; o += kWave * 16) {
        const Bytes16 v = load16(text, nbytes, a + o, aligned);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)v.b[k] << (8 * (k & 3));
        *reinterpret_cast<uint4*>(stage + o) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
  __syncthreads();
  const int64_t i = r0 + lane;
  bool bad = false;
  if (i < r1) {
    const int64_t s = row_start[i], e = row_start[i + 1];
    if (s > e || e > nbytes || e - s > kRowMaxBytes)
      bad = true;
    else if (staged && s >= lo && e <= hi)
      bad = !parse_row(stage + (s - a), (int)(e - s), n_cols, n_rows, i, out);
    else
      bad = !parse_row(text + s, (int)(e - s), n_cols, n_rows, i, out);
  }
  const uint64_t m = __ballot(bad);
  if (m && lane == 0) atomicAdd(n_bad, (unsigned long long)__popcll(m));
}
}  // namespace

int64_t text_tile_bytes() { return kTileBytes; }

int32_t text_rows_index(const uint8_t* text, int64_t nbytes, int64_t n_rows, uint32_t* row_start,
                        int64_t* lines_found_host, int64_t* n_bad_host, hipStream_t st) {
  *lines_found_host = 0;
  *n_bad_host = 0;
  // entries no '\n' reaches stay past every nbytes: k_parse counts their rows as unsupported
  RPT_HIP(hipMemsetAsync(row_start, 0xff, sizeof(uint32_t) * (size_t)(n_rows + 1), st));
  if (nbytes == 0) {
    RPT_HIP(hipMemsetAsync(row_start, 0, sizeof(uint32_t), st));
    return wait_stream(st);
  }
  const int64_t n_tiles = (nbytes + kTileBytes - 1) / kTileBytes;
  Scratch& sc = scratch(st);
  Budget bud;
  bud.add<int32_t>(n_tiles);
  bud.add<int64_t>(n_tiles + 1);
  RPT_TRY(sc.reserve(bud.bytes, st));
  int32_t* tile_lines = sc.carve_n<int32_t>(n_tiles);
  int64_t* tile_base = sc.carve_n<int64_t>(n_tiles + 1);
  unsigned long long* n_bad = nullptr;
  RPT_TRY(zero_n(st, 1, &n_bad));
  const dim3 grid((unsigned)n_tiles);
  hipLaunchKernelGGL(k_count, grid, dim3(kBlock), 0, st, text, nbytes, tile_lines, n_bad);
  RPT_CHECK_LAUNCH();
  RPT_TRY(exclusive_scan_total_i32_to_i64(tile_lines, tile_base, n_tiles, st));
  hipLaunchKernelGGL(k_starts, grid, dim3(kBlock), 0, st, text, nbytes, tile_base, n_tiles,
                     n_rows, row_start);
  RPT_CHECK_LAUNCH();
  int64_t newlines = 0;
  unsigned long long bad = 0;
  uint8_t last = 0;
  RPT_HIP(hipMemcpyAsync(&newlines, tile_base + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost,
                         st));
  RPT_HIP(hipMemcpyAsync(&bad, n_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  RPT_HIP(hipMemcpyAsync(&last, text + nbytes - 1, 1, hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  *lines_found_host = newlines + (last != '\n');  // a last line without '\n' is a line
  *n_bad_host = (int64_t)bad;
  return RPT_OK;
}

int32_t text_rows_parse(const uint8_t* text, int64_t nbytes, const uint32_t* row_start,
                        int64_t n_rows, int32_t n_cols, float* out, int64_t* n_bad_host,
                        hipStream_t st) {
  *n_bad_host = 0;
  if (n_rows == 0) return wait_stream(st);
  unsigned long long* n_bad = nullptr;
  RPT_TRY(zero_n(st, 1, &n_bad));
  const dim3 grid((unsigned)((n_rows + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(k_parse, grid, dim3(kBlock), 0, st, text, nbytes, row_start, n_rows,
                     (int)n_cols, out, n_bad);
  RPT_CHECK_LAUNCH();
  unsigned long long bad = 0;
  RPT_HIP(hipMemcpyAsync(&bad, n_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  RPT_TRY(wait_stream(st));
  *n_bad_host = (int64_t)bad;
  return RPT_OK;
}

}  // namespace rpt
