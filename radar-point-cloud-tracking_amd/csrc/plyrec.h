// Per-value code of the denoise pipeline's PLY writer (write_ply,
// PointCloudWorkF/stdbscan_denoising_pipeline.py:767-855), one routine each for the device
// (csrc/plyrec.hip) and the host (rpt_ply_records_host in csrc/plyrec.cpp,
// tools/asan/plyrec_main.cpp):
//
//   plyrec::keep            which points a file holds: all of them, or labels[i] >= 0
//   plyrec::viridis_index   the colormap row of an intensity, as matplotlib's Colormap.__call__
//                           evaluates viridis(np.clip(z / 255.0, 0, 1)) on a float32 array
//   plyrec::color           the point's colour from the LUT of its mode
//   plyrec::words           the 15-byte record as four little-endian words (top byte zero)
//
// Every float operation is a single float32 operation rounded once; the division is an IEEE
// division (heat::fdiv), the multiply by 256 is exact.
#pragma once
#include <stdint.h>

#include "heat.h"

namespace rpt {
namespace plyrec {

constexpr int kRecord = 15;        // x, y, z float32 little-endian, then r, g, b
constexpr int kTile = 1024;        // points of one tile of the size / write passes
constexpr int kTabColors = 20;     // rows of the label LUT (tab20)
constexpr int kViridisBad = 256;   // row of the intensity LUT a NaN takes; rows 0..255 the map
constexpr int kNoiseGrey = 128;

RPT_HEAT_HD bool keep(bool has_labels, bool signal_only, int32_t label) {
  return !has_labels || !signal_only || label >= 0;
}

// zn = clip(z / 255, 0, 1); f = zn * 256; f == 256 -> 255, else int(f).  np.clip is
// minimum(maximum(zn, 0), 1): a NaN stays a NaN and takes the map's "bad" row, -inf gives row 0
// and +inf row 255 through the clip, -0.0 gives row 0.
RPT_HEAT_HD int viridis_index(float z) {
  float zn = heat::fdiv(z, 255.0f);
  if (zn != zn) return kViridisBad;
  if (zn < 0.0f) zn = 0.0f;
  if (zn > 1.0f) zn = 1.0f;
  const float f = zn * 256.0f;
  return f == 256.0f ? 255 : (int)f;
}

// lut: [20][3] with labels (label % 20; any negative label grey), [257][3] without
RPT_HEAT_HD uint32_t color(const uint8_t* lut, bool has_labels, int32_t label, float z) {
  int row;
  if (has_labels) {
    if (label < 0) return (uint32_t)kNoiseGrey * 0x010101u;
    row = (int)((uint32_t)label % (uint32_t)kTabColors);
  } else {
    row = viridis_index(z);
  }
  const uint8_t* c = lut + 3 * row;
  return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
}

// The record's bytes 4k .. 4k + 3 as the little-endian word w[k]; the coordinates' bit patterns
// go through unchanged (NaN payloads included), rgb is color()'s packing.
RPT_HEAT_HD void words(float x, float y, float z, uint32_t rgb, uint32_t w[4]) {
  w[0] = heat::f2u(x);
  w[1] = heat::f2u(y);
  w[2] = heat::f2u(z);
  w[3] = rgb & 0xffffffu;
}

}  // namespace plyrec
}  // namespace rpt
