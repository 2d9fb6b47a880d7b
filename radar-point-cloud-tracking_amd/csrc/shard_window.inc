// Shard driver, the halo exchange's two ends.  Reads shard_shared.inc (kHaloHdr, halo_total,
// WinMeta) and common.h (BoundsAcc).
//   rpt_shard_halo    k_halo_pack: reads the own kept x / y / frame slots and the kept frame
//                     offsets, leaves the first and last hf frames' points in the two send buffers
//   rpt_shard_window  ONE of, then stdbscan_bounds_final_dev over the partials:
//                     k_window (land filter off): reads both received halos and the own points,
//                     leaves the window's X / Y / T from index 0, WinMeta, one Bounds partial per
//                     block;
//                     k_window_halo (land filter on: the compaction already wrote the own points
//                     at own_off): places the halos around them, leaves WinMeta, the halo points'
//                     partials and, as partial nb, the own points' bounds from the compaction

// The own edge frames for the neighbours: {count, own kept total (lo, hi), 0} then x, y and
// t = frame0 + slot (float32 bits) at fixed offsets of the buffer's capacity (the K1 count of
// those frames, which the land filter can only shrink).
__global__ void k_halo_pack(const float* __restrict__ x, const float* __restrict__ y,
                            const int32_t* __restrict__ pf, const int64_t* __restrict__ off,
                            int32_t F, int32_t hf, int64_t frame0, int32_t* __restrict__ sp,
                            int64_t cap_p, int32_t* __restrict__ sn, int64_t cap_n) {
  const int64_t K = off[F];
  const int64_t nh = min(off[hf], cap_p);
  const int64_t t0 = off[F - hf];
  const int64_t nt = min(K - t0, cap_n);
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (i0 == 0) {
    if (sp) {
      sp[0] = (int32_t)nh;
      sp[1] = (int32_t)(uint32_t)(uint64_t)K;
      sp[2] = (int32_t)(uint32_t)((uint64_t)K >> 32);
      sp[3] = 0;
    }
    if (sn) {
      sn[0] = (int32_t)nt;
      sn[1] = (int32_t)(uint32_t)(uint64_t)K;
      sn[2] = (int32_t)(uint32_t)((uint64_t)K >> 32);
      sn[3] = 0;
    }
  }
  if (sp)
    for (int64_t i = i0; i < nh; i += step) {
      sp[kHaloHdr + i] = __float_as_int(x[i]);
      sp[kHaloHdr + cap_p + i] = __float_as_int(y[i]);
      sp[kHaloHdr + 2 * cap_p + i] = __float_as_int((float)(frame0 + (int64_t)pf[i]));
    }
  if (sn)
    for (int64_t i = i0; i < nt; i += step) {
      const int64_t j = t0 + i;
      sn[kHaloHdr + i] = __float_as_int(x[j]);
      sn[kHaloHdr + cap_n + i] = __float_as_int(y[j]);
      sn[kHaloHdr + 2 * cap_n + i] = __float_as_int((float)(frame0 + (int64_t)pf[j]));
    }
}

// [prev halo | own | next halo] as x / y / t, the window's counts, and per block the partial of
// the window's ST-DBSCAN bounds (k_bounds' semantics, reduced by stdbscan_bounds_final_dev: no
// separate bounds pass over the window)
__global__ __launch_bounds__(kBoundsBlock) void k_window(
    const int32_t* __restrict__ rp, int64_t cap_rp, const int32_t* __restrict__ rn,
    int64_t cap_rn, const float* __restrict__ x, const float* __restrict__ y,
    const int32_t* __restrict__ pf, const int64_t* __restrict__ off, int32_t F, int32_t hf,
    int64_t frame0, float* __restrict__ X, float* __restrict__ Y, float* __restrict__ T,
    WinMeta* __restrict__ meta, Bounds* __restrict__ part) {
  const int64_t np = rp ? (int64_t)rp[0] : 0;
  const int64_t nn = rn ? (int64_t)rn[0] : 0;
  const int64_t K = off[F];
  const int64_t total = np + K + nn;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) {
    WinMeta m;
    m.n_prev = np;
    m.n_own = K;
    m.n_next = nn;
    m.k_prev_total = rp ? halo_total(rp) : 0;
    m.n_head = off[hf];
    m.n_tail = K - off[F - hf];
    m.n_window = total;
    m.pad = 0;
    *meta = m;
  }
  auto time_of = [&](int64_t i) -> float {
    if (i < np) return __int_as_float(rp[kHaloHdr + 2 * cap_rp + i]);
    if (i < np + K) return (float)(frame0 + (int64_t)pf[i - np]);
    return __int_as_float(rn[kHaloHdr + 2 * cap_rn + (i - np - K)]);
  };
  BoundsAcc acc;
  for (int64_t i = i0; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float a, b, c;
    if (i < np) {
      a = __int_as_float(rp[kHaloHdr + i]);
      b = __int_as_float(rp[kHaloHdr + cap_rp + i]);
      c = __int_as_float(rp[kHaloHdr + 2 * cap_rp + i]);
    } else if (i < np + K) {
      const int64_t j = i - np;
      a = x[j];
      b = y[j];
      c = (float)(frame0 + (int64_t)pf[j]);
    } else {
      const int64_t j = i - np - K;
      a = __int_as_float(rn[kHaloHdr + j]);
      b = __int_as_float(rn[kHaloHdr + cap_rn + j]);
      c = __int_as_float(rn[kHaloHdr + 2 * cap_rn + j]);
    }
    X[i] = a;
    Y[i] = b;
    T[i] = c;
    acc.add(a, b, c, i > 0 ? time_of(i - 1) : 0.f, i > 0);
  }
  acc.block_store(part);
}

// The direct window (the land compaction already wrote the own points at own_off): the halo
// points placed around them -- prev halo at [own_off - np, own_off), next halo at
// [own_off + K, own_off + K + nn) -- the window's counts, and per block the partial of the halo
// points' bounds (k_window's semantics: every point's time against its window predecessor's);
// partial nb is the own points' bounds from the compaction, with the prev halo -> own junction
// folded in, so k_bounds_final over nb + 1 partials gives the window's bounds.
__global__ __launch_bounds__(kBoundsBlock) void k_window_halo(
    const int32_t* __restrict__ rp, int64_t cap_rp, const int32_t* __restrict__ rn,
    int64_t cap_rn, const int64_t* __restrict__ off, int32_t F, int32_t hf, int64_t own_off,
    float* __restrict__ X, float* __restrict__ Y, float* __restrict__ T,
    WinMeta* __restrict__ meta, Bounds* __restrict__ part, int nb,
    const Bounds* __restrict__ own_bnd) {
  const int64_t np = rp ? (int64_t)rp[0] : 0;
  const int64_t nn = rn ? (int64_t)rn[0] : 0;
  const int64_t K = off[F];
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0) {
    WinMeta m;
    m.n_prev = np;
    m.n_own = K;
    m.n_next = nn;
    m.k_prev_total = rp ? halo_total(rp) : 0;
    m.n_head = off[hf];
    m.n_tail = K - off[F - hf];
    m.n_window = np + K + nn;
    m.pad = 0;
    *meta = m;
    Bounds o = *own_bnd;
    if (np > 0 && K > 0 && !(__int_as_float(rp[kHaloHdr + 2 * cap_rp + np - 1]) <= T[own_off]))
      o.t_descends = 1;  // (NaN counts as out of order, as in BoundsAcc)
    part[nb] = o;
  }
  BoundsAcc acc;
  for (int64_t h = i0; h < np + nn; h += (int64_t)gridDim.x * blockDim.x) {
    float a, b, c, tp;
    bool hp;
    if (h < np) {
      a = __int_as_float(rp[kHaloHdr + h]);
      b = __int_as_float(rp[kHaloHdr + cap_rp + h]);
      c = __int_as_float(rp[kHaloHdr + 2 * cap_rp + h]);
      const int64_t i = own_off - np + h;
      X[i] = a;
      Y[i] = b;
      T[i] = c;
      hp = h > 0;
      tp = hp ? __int_as_float(rp[kHaloHdr + 2 * cap_rp + h - 1]) : 0.f;
    } else {
      const int64_t j = h - np;
      a = __int_as_float(rn[kHaloHdr + j]);
      b = __int_as_float(rn[kHaloHdr + cap_rn + j]);
      c = __int_as_float(rn[kHaloHdr + 2 * cap_rn + j]);
      const int64_t i = own_off + K + j;
      X[i] = a;
      Y[i] = b;
      T[i] = c;
      // predecessor: the next halo's previous point, else the last own point, else the last
      // prev halo point
      hp = j > 0 || K > 0 || np > 0;
      tp = j > 0 ? __int_as_float(rn[kHaloHdr + 2 * cap_rn + j - 1])
                 : (K > 0 ? T[own_off + K - 1]
                          : (np > 0 ? __int_as_float(rp[kHaloHdr + 2 * cap_rp + np - 1]) : 0.f));
    }
    acc.add(a, b, c, tp, hp);
  }
  acc.block_store(part);
}
