// K1 on generic sweeps (f32 echo, any bin count, unaligned u8): one wave per row.  Launched by
// count_impl (k_row_count, k_file_counts) and write_impl (k_row_write) of polar.hip when the
// stack does not take the grouped u8 kernels.
//   k_row_count    reads the echo; leaves one kept count per ROW (the driver scans them into
//                  row_prefix, n_files * rows + 1 values)
//   k_file_counts  reads row_prefix; leaves per file ceil(kept / stride) (the driver scans them
//                  into file_offsets, n_files + 1 values, the last one the total)
//   k_row_write    reads the echo again, row_prefix, file_offsets and the rows' geometry (RowGeo:
//                  per-row scale or per-sample ranges); writes x, y, val, gain and point frame of
//                  every stride-th kept sample of each file.  No staged entries, no bounds.
// Reads polar_shared.inc (Vec, to_f, wave_excl_scan) and common.h (rank_in_mask).

// Row pass: count kept elements per row.  VEC path needs bins % (64*N) == 0 and aligned rows.
template <class T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_row_count(const T* __restrict__ echo,
                                                     int64_t n_rows, int bins, float thr,
                                                     int32_t* __restrict__ row_count) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / 64;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t row = wave0; row < n_rows; row += n_waves) {
    const T* rp = echo + row * bins;
    int c = 0;
    if (VEC) {
      constexpr int N = Vec<T>::N;
      using L = typename Vec<T>::L;
      for (int b0 = lane * N; b0 < bins; b0 += 64 * N) {
        const L v = *reinterpret_cast<const L*>(rp + b0);
        float f[N];
        Vec<T>::unpack(v, f);
#pragma unroll
        for (int k = 0; k < N; ++k) c += (f[k] > thr) ? 1 : 0;
      }
    } else {
      for (int b = lane; b < bins; b += 64) c += (to_f(rp[b]) > thr) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) row_count[row] = c;
  }
}

// file_offsets[f] = sum over earlier files of ceil(kept / stride); kept from row_prefix.
__global__ void k_file_counts(const int64_t* __restrict__ row_prefix, int64_t n_files, int rows,
                              int stride, int64_t* __restrict__ file_out) {
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_files;
       f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kept = row_prefix[(f + 1) * rows] - row_prefix[f * rows];
    file_out[f] = (kept + stride - 1) / stride;
  }
}

struct RowGeo {
  const float* scale;   // per row (scale mode) or nullptr
  const float* ranges;  // [row][bin] (ranges mode) or nullptr
  const float* cos_t;
  const float* sin_t;
};

// Row pass 2: write the kept elements whose in-file rank is a multiple of stride.  Each lane ranks
// its kept elements, the emitted ones (bin, value) are staged in the wave's LDS slice in output
// order, and the wave then writes them with full-width coalesced stores (a row emits only
// ~kept/stride points, so storing from the ranking lanes directly would issue ~5 x 16 mostly
// masked store instructions per row).
template <class T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_row_write(
    const T* __restrict__ echo, int64_t n_rows, int rows, int bins, float thr, int stride,
    RowGeo geo, const int32_t* __restrict__ gain, const int64_t* __restrict__ row_prefix,
    const int64_t* __restrict__ file_offsets, int files_per_frame, float* __restrict__ x,
    float* __restrict__ y, float* __restrict__ val, int32_t* __restrict__ gain_out,
    int32_t* __restrict__ pf_out) {
  constexpr int CH = VEC ? 64 * Vec<T>::N : 64;  // bins per chunk
  __shared__ uint16_t s_bin[kWavesPerBlock][CH];
  __shared__ float s_val[kWavesPerBlock][CH];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x / 64;
  const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + wv;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
  const float fb = (float)bins;
  const uint32_t ustride = (uint32_t)stride;
  for (int64_t row = wave0; row < n_rows; row += n_waves) {
    const int64_t f = (int64_t)((uint32_t)row / (uint32_t)rows);  // n_rows < 2^32 (host check)
    const T* rp = echo + row * bins;
    // in-file rank of this row's first kept element (< rows*bins, fits 32 bits)
    uint32_t rank = (uint32_t)(row_prefix[row] - row_prefix[f * rows]);
    const int64_t out0 = file_offsets[f];
    const float step = geo.scale ? geo.scale[row] / fb : 0.f;
    const float ct = geo.cos_t[row], st = geo.sin_t[row];
    const int32_t g = gain ? gain[f] : 0;
    const int32_t fr = (int32_t)((uint32_t)f / (uint32_t)files_per_frame);
    for (int base = 0; base < bins; base += CH) {
      int tot;
      if (VEC) {
        constexpr int N = Vec<T>::N;
        using L = typename Vec<T>::L;
        const int b0 = base + lane * N;
        const L v = *reinterpret_cast<const L*>(rp + b0);
        float fv[N];
        Vec<T>::unpack(v, fv);
        int c = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) c += (fv[k] > thr) ? 1 : 0;
        const uint32_t r = rank + (uint32_t)wave_excl_scan(c, &tot);
        if (c) {
          // emitted = kept elements with in-file rank % stride == 0: one 32-bit division per
          // lane, then a countdown; slot = output index - the chunk's first output index
          const uint32_t q = r / ustride, rem = r - q * ustride;
          uint32_t skip = rem ? ustride - rem : 0u;
          int slot = (int)(q + (rem ? 1u : 0u) - (rank + ustride - 1u) / ustride);
#pragma unroll
          for (int k = 0; k < N; ++k) {
            if (fv[k] > thr) {
              if (skip == 0u) {
                s_bin[wv][slot] = (uint16_t)(b0 + k - base);
                s_val[wv][slot] = fv[k];
                ++slot;
                skip = ustride - 1u;
              } else {
                --skip;
              }
            }
          }
        }
      } else {
        const int b = base + lane;
        const float v = (b < bins) ? to_f(rp[b]) : 0.f;
        const bool keep = (b < bins) && (v > thr);
        const uint64_t m = __ballot(keep);
        tot = __popcll(m);
        if (keep) {
          const uint32_t r = rank + (uint32_t)rank_in_mask(m);
          const uint32_t q = r / ustride;
          if (r - q * ustride == 0u) {
            const int slot = (int)(q - (rank + ustride - 1u) / ustride);
            s_bin[wv][slot] = (uint16_t)lane;
            s_val[wv][slot] = v;
          }
        }
      }
      const uint32_t first = (rank + ustride - 1u) / ustride;
      const int n_emit = (int)((rank + (uint32_t)tot + ustride - 1u) / ustride - first);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int l = lane; l < n_emit; l += 64) {
        const int b = base + (int)s_bin[wv][l];
        const int64_t o = out0 + first + l;
        const float rr = geo.ranges ? geo.ranges[row * bins + b] : step * (float)b;
        x[o] = rr * ct;
        y[o] = rr * st;
        val[o] = s_val[wv][l];
        if (gain_out) gain_out[o] = g;
        if (pf_out) pf_out[o] = fr;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      rank += (uint32_t)tot;
    }
  }
}
