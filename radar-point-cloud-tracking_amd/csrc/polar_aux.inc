// Small kernels beside K1, each launched by the C-ABI body of polar.hip named here; none reads
// or leaves anything of the K1 stages.
//   k_frame_times     frame_times, frame_times_dev   point frame slot -> float time (or its id)
//   k_frame_fill      frame_fill                     frame offsets -> per-point time and slot
//   k_bytes_to_float  bytes_to_float                 out[i] = (float)in[i]
//   k_polar_dense     polar_to_cartesian             every sample of one sweep to x, y
//   k_colors          infer_time_from_colors         nearest palette entry per point
//   k_synth           synth_echo                     the synthetic echo (rpt/synth.py numpy_echo)
// Reads polar_shared.inc (kBlock) only.

__global__ void k_frame_times(const int32_t* __restrict__ pf, int64_t n,
                              const int64_t* __restrict__ ids, float* __restrict__ t,
                              const int64_t* __restrict__ n_dev) {
  if (n_dev) n = *n_dev;  // count on the device (at most the host n the grid was sized for)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t f = pf[i];
    t[i] = (float)(ids ? ids[f] : (int64_t)f);
  }
}

// frame slots from frame offsets: block f fills the points [off[f], off[f + 1]) of frame f
__global__ void k_frame_fill(const int64_t* __restrict__ off, float* __restrict__ t,
                             int32_t* __restrict__ pf) {
  const int32_t f = blockIdx.x;
  const int64_t hi = off[f + 1];
  for (int64_t i = off[f] + threadIdx.x; i < hi; i += blockDim.x) {
    if (t) t[i] = (float)f;
    if (pf) pf[i] = f;
  }
}

__global__ void k_bytes_to_float(const uint8_t* __restrict__ in, int64_t n,
                                 float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}

__global__ void k_polar_dense(const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                              const float* __restrict__ ranges, int64_t rows, int64_t bins,
                              float* __restrict__ x, float* __restrict__ y) {
  const int64_t n = rows * bins;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / bins;
    const float rr = ranges[i];
    x[i] = rr * cos_t[r];
    y[i] = rr * sin_t[r];
  }
}

// ---------------------------------------------------------------- colour -> time
// clustering.py:39-46: diffs f32, dist2 = ((d0*d0) + d1*d1) + d2*d2, first argmin.
__global__ void k_colors(const uint8_t* __restrict__ colors, int64_t n,
                         const float* __restrict__ pal, int n_pal, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float r = colors[3 * i], g = colors[3 * i + 1], b = colors[3 * i + 2];
    int best = 0;
    float bd = 0.f;
    for (int k = 0; k < n_pal; ++k) {
      const float d0 = r - pal[3 * k], d1 = g - pal[3 * k + 1], d2 = b - pal[3 * k + 2];
      float d = d0 * d0;
      d = d + d1 * d1;
      d = d + d2 * d2;
      // np.argmin: first minimum; a NaN wins immediately (cannot occur for u8 colours)
      if (k == 0 || d < bd) {
        bd = d;
        best = k;
      }
    }
    out[i] = (float)best;
  }
}

// ---------------------------------------------------------------- synthetic echo
// Bit-identical restatement: rpt/synth.py::numpy_echo.
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int kMaxTargets = 256;

// One block per (frame, gain, row); threads sweep the bins.
__global__ __launch_bounds__(kBlock) void k_synth(rpt_synth_params p, int64_t frame0,
                                                 int64_t n_frames, const float* __restrict__ cos_t,
                                                 const float* __restrict__ sin_t,
                                                 const uint32_t* __restrict__ clutter_thresh,
                                                 const float* __restrict__ targets,
                                                 const int32_t* __restrict__ trows,
                                                 const int32_t* __restrict__ tbins,
                                                 uint8_t* __restrict__ echo) {
  __shared__ int hits[kMaxTargets];
  __shared__ int n_hits;
  const int64_t n_rows_total = n_frames * p.n_gains * p.rows;
  for (int64_t rr = blockIdx.x; rr < n_rows_total; rr += gridDim.x) {
    const int row = (int)(rr % p.rows);
    const int64_t fg = rr / p.rows;
    const int gi = (int)(fg % p.n_gains);
    const int64_t fl = fg / p.n_gains;  // local frame
    const int64_t fa = frame0 + fl;      // absolute frame (hash input)
    __syncthreads();
    if (threadIdx.x == 0) n_hits = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < p.n_targets; k += blockDim.x) {
      const int32_t* tr = trows + (fl * p.n_targets + k) * 2;
      if (row >= tr[0] && row <= tr[1]) hits[atomicAdd(&n_hits, 1)] = k;
    }
    __syncthreads();
    const int nh = n_hits;
    // deterministic target order: insertion sort of the (few) hits
    if (threadIdx.x == 0) {
      for (int a = 1; a < nh; ++a) {
        const int v = hits[a];
        int b = a - 1;
        while (b >= 0 && hits[b] > v) {
          hits[b + 1] = hits[b];
          --b;
        }
        hits[b + 1] = v;
      }
    }
    __syncthreads();
    const float step = p.scale / (float)p.bins;
    const float ct = cos_t[row], st = sin_t[row];
    const bool land_row = row >= p.land_row0 && row < p.land_row1;
    uint8_t* out = echo + rr * p.bins;
    for (int b = threadIdx.x; b < p.bins; b += blockDim.x) {
      const uint64_t idx = (((uint64_t)(fa * p.n_gains + gi) * (uint64_t)p.rows + row) *
                            (uint64_t)p.bins) + (uint64_t)b;
      const uint64_t h = splitmix64(p.seed ^ (idx * 0xD1B54A32D192ED03ull));
      uint32_t v = 0;
      if ((uint32_t)(h >> 32) < clutter_thresh[gi * p.bins + b]) v = 11u + (uint32_t)((h >> 16) & 0xffffu) % 29u;
      if (land_row && b >= p.land_bin0 && (uint32_t)(h & 0xffu) < p.land_fill_u8)
        v = 150u + (uint32_t)((h >> 8) & 0xffu) % 106u;
      if (nh) {
        const float r = step * (float)b;
        const float xx = r * ct, yy = r * st;
        for (int q = 0; q < nh; ++q) {
          const int k = hits[q];
          const int32_t* tb = tbins + (fl * p.n_targets + k) * 2;
          if (b < tb[0] || b > tb[1]) continue;
          const float* tg = targets + (fl * p.n_targets + k) * 4;
          const float dx = xx - tg[0], dy = yy - tg[1];
          float d2 = dx * dx;
          d2 = d2 + dy * dy;
          if (d2 <= tg[2]) {
            if ((uint32_t)((h >> 40) & 0xffu) < p.target_fill_u8)
              v = 60u + (uint32_t)((h >> 48) & 0xffu) % 40u;
            break;
          }
        }
      }
      out[b] = (uint8_t)v;
    }
  }
}
