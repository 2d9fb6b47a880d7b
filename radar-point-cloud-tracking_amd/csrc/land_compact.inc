// K3 fused compaction of the stack driver, launched by land_compact_dev of land.hip in this order:
//   k_land_tile_counts<CT>  reads cell, land -> tile_cnt[tile], each tile's kept points
//   (exclusive_scan_total_i32: tile_cnt -> base, base[nt] = the kept count)
//   k_land_compact<OFFS, CT, VT>  reads the points, cell, land, base -> the kept points in order
//                           (xo, yo, vo, go, pfo), their times to, and part[tile], the tile's
//                           share of the ST-DBSCAN bounds.  OFFS: frames from frame_off, no pf
//   k_land_new_off          (with pf) base[nt], pfo -> new_off[0 .. n_frames]
//   k_land_new_off_tiles<CT>  (with frame_off) base, cell, land, frame_off -> new_off
//   k_land_compact_final    part, base[nt] -> *bounds_out
// Reads land_shared.inc (f2ord) and frame_index.h.

// ---- fused compaction of the stack driver (filter_land_from_frame, :426-436, over the stack) --
// Tiles of kCompTile points; item k of thread t is point tile*kCompTile + k*kCompBlock + t, so
// loads and (kept-order) stores are coalesced.  Pass 1 counts each tile's kept points (cell not
// land) from the cells the grid pass stored; after a scan of the tile counts, pass 2 recomputes
// the flags, ranks them (ballots + a 64-entry scan of the per-(item, wave) counts) and writes the
// kept points in order with their times (float32 frame slots, :460-467) and a per-tile partial of
// the ST-DBSCAN bounds -- the keep / position arrays, their full-length scan, the frame-time
// pass and the bounds pass of the separate kernels are gone.
constexpr int kCompBlock = 256, kCompItems = 16, kCompTile = kCompBlock * kCompItems;

struct BoundsPart {
  uint32_t mnx, mxx, mny, mxy;
  int32_t mnf, mxf, flags, pad;  // flags: 1 non-finite x/y, 2 frame slots descend
};

template <class CT>
__global__ __launch_bounds__(kCompBlock) void k_land_tile_counts(const CT* __restrict__ cell,
                                                                int64_t n,
                                                                const uint8_t* __restrict__ land,
                                                                int32_t* __restrict__ tile_cnt) {
  int32_t cl[kCompItems];
  if constexpr (sizeof(CT) == 2) {
    // 16-bit cells: a thread takes 16 consecutive cells as two 16-B loads (the count does not
    // depend on which thread sees which point; 2-B loads, 128 B per wave instruction, were
    // slower than the int32 form's: 68 against 50 us at 1000 frames)
    static_assert(kCompItems == 16, "two uint4 loads of eight 16-bit cells each");
    const int64_t b = (int64_t)blockIdx.x * kCompTile + (int64_t)threadIdx.x * kCompItems;
    if (b + kCompItems <= n) {
      const uint4* p = reinterpret_cast<const uint4*>(cell + b);  // (tiles start 8 KiB apart)
      const uint4 lo = p[0], hi = p[1];
      const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        cl[2 * q] = (int32_t)(w[q] & 0xffffu);
        cl[2 * q + 1] = (int32_t)(w[q] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCompItems; ++k) cl[k] = (b + k < n) ? (int32_t)cell[b + k] : -1;
    }
  } else {
    const int64_t i0 = (int64_t)blockIdx.x * kCompTile + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCompItems; ++k) {
      const int64_t i = i0 + (int64_t)k * kCompBlock;
      cl[k] = (i < n) ? cell[i] : -1;
    }
  }
  uint32_t lnd[kCompItems];  // branch-free: the flags' loads in flight together (>= 1 cell)
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) lnd[k] = land[cl[k] >= 0 ? cl[k] : 0];
  int c = 0;
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) c += (cl[k] >= 0 && !lnd[k]) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  __shared__ int ws[kCompBlock / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kCompBlock / 64; ++w) t += ws[w];
    tile_cnt[blockIdx.x] = t;
  }
}

// OFFS (the stack driver's narrow path): no per-point frame slots in or out (pf, pfo unused);
// a point's frame comes from the frame offsets fo[0 .. F] of the input (frame_index.h): one
// search for the frame of the tile's first point, then one wave-uniform step per offset that
// falls inside the tile (usually none or one; any number, runs of empty frames included).
// CT, VT: the cells' and the intensities' element types (see the grid kernels; v is only copied).
template <bool OFFS, class CT, class VT>
__global__ __launch_bounds__(kCompBlock) void k_land_compact(
    const float* __restrict__ x, const float* __restrict__ y, const VT* __restrict__ v,
    const int32_t* __restrict__ g, const int32_t* __restrict__ pf, int64_t n,
    const CT* __restrict__ cell, const uint8_t* __restrict__ land,
    const int32_t* __restrict__ tile_base, float* __restrict__ xo, float* __restrict__ yo,
    VT* __restrict__ vo, int32_t* __restrict__ go, int32_t* __restrict__ pfo,
    float* __restrict__ to, BoundsPart* __restrict__ part, int64_t t_base,
    const int64_t* __restrict__ fo, int F) {
  constexpr int NW = kCompBlock / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int64_t i0 = (int64_t)blockIdx.x * kCompTile + threadIdx.x;
  int32_t cl[kCompItems];
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) {
    const int64_t i = i0 + (int64_t)k * kCompBlock;
    cl[k] = (i < n) ? cell[i] : -1;
  }
  // every load below is branch-free (clamped index, result masked) so a thread's loads of a batch
  // are in flight together: conditional loads each ended in a full vmcnt wait
  uint32_t lnd[kCompItems];
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) lnd[k] = land[cl[k] >= 0 ? cl[k] : 0];  // >= 1 cell
  uint32_t km = 0;
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) km |= (cl[k] >= 0 && !lnd[k]) ? (1u << k) : 0u;
  __shared__ int cw[kCompItems * NW];  // per (item k, wave) counts, then their exclusive scan
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) {
    const uint64_t bk = __ballot((km >> k) & 1u);
    if (lane == 0) cw[k * NW + w] = __popcll(bk);
  }
  __syncthreads();
  static_assert(kCompItems * NW == 64, "one wave scans the per-(item, wave) counts");
  if (w == 0) {
    const int c = cw[lane];
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    cw[lane] = incl - c;
  }
  __syncthreads();
  const int64_t tb = tile_base[blockIdx.x];
  uint32_t mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u;
  int mnf = INT_MAX, mxf = INT_MIN, flags = 0;
  const int64_t tile_lo = (int64_t)blockIdx.x * kCompTile;  // < n: the grid is ceil(n / tile)
  const int64_t tile_hi = min(tile_lo + kCompTile, n);
  int f0 = 0;  // (block-uniform) frame of the tile's first point
  if constexpr (OFFS) f0 = __builtin_amdgcn_readfirstlane(frame_of_point(fo, F, tile_lo));
  constexpr int kB = 4;  // items per batch of loads
#pragma unroll
  for (int k0 = 0; k0 < kCompItems; k0 += kB) {
    int fb[kB], fp[kB], gb[kB];
    float xb[kB], yb[kB];
    VT vb[kB];
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      const int64_t i = min(i0 + (int64_t)(k0 + u) * kCompBlock, n - 1);
      if constexpr (OFFS) {
        fb[u] = f0;
        fp[u] = 0;
      } else {
        fb[u] = pf[i];
        fp[u] = pf[i > 0 ? i - 1 : 0];
      }
      xb[u] = x[i];
      yb[u] = y[i];
      vb[u] = v[i];
      gb[u] = go ? g[i] : 0;
    }
    if constexpr (OFFS) {
      // frame = f0 + the offsets after fo[f0] that are <= i; those inside the tile are the only
      // ones that can be (fo ascends: the loop ends at the first one at or past the tile's end)
      for (int q = f0 + 1; q < F; ++q) {
        const int64_t o = fo[q];  // (uniform)
        if (o >= tile_hi) break;
#pragma unroll
        for (int u = 0; u < kB; ++u)
          fb[u] += (i0 + (int64_t)(k0 + u) * kCompBlock >= o) ? 1 : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < kB; ++u) {
    const int k = k0 + u;
    const int64_t i = i0 + (int64_t)k * kCompBlock;
    const bool kp = (km >> k) & 1u;
    const uint64_t bk = __ballot(kp);
    if (i < n) {
      const int f = fb[u];
      // input order; the kept points descend only if the input does (OFFS: frames from
      // ascending offsets cannot descend by construction, the flag stays clear)
      if (!OFFS && i > 0 && f < fp[u]) flags |= 2;
      if (kp) {
        const int64_t o = tb + cw[k * NW + w] + __popcll(bk & lt);
        const float px = xb[u], py = yb[u];
        xo[o] = px;
        yo[o] = py;
        vo[o] = vb[u];
        if (go) go[o] = gb[u];
        if constexpr (!OFFS) pfo[o] = f;
        to[o] = (float)(t_base + (int64_t)f);  // (t_base: the shard driver's first frame)
        if (!isfinite(px) || !isfinite(py)) flags |= 1;
        const uint32_t a = f2ord(px), b = f2ord(py);
        mnx = min(mnx, a);
        mxx = max(mxx, a);
        mny = min(mny, b);
        mxy = max(mxy, b);
        mnf = min(mnf, f);
        mxf = max(mxf, f);
      }
    }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mnx = min(mnx, (uint32_t)__shfl_xor((int)mnx, off));
    mxx = max(mxx, (uint32_t)__shfl_xor((int)mxx, off));
    mny = min(mny, (uint32_t)__shfl_xor((int)mny, off));
    mxy = max(mxy, (uint32_t)__shfl_xor((int)mxy, off));
    mnf = min(mnf, __shfl_xor(mnf, off));
    mxf = max(mxf, __shfl_xor(mxf, off));
    flags |= __shfl_xor(flags, off);
  }
  __shared__ BoundsPart wp[NW];
  if (lane == 0) wp[w] = BoundsPart{mnx, mxx, mny, mxy, mnf, mxf, flags, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    BoundsPart r = wp[0];
    for (int q = 1; q < NW; ++q) {
      r.mnx = min(r.mnx, wp[q].mnx);
      r.mxx = max(r.mxx, wp[q].mxx);
      r.mny = min(r.mny, wp[q].mny);
      r.mxy = max(r.mxy, wp[q].mxy);
      r.mnf = min(r.mnf, wp[q].mnf);
      r.mxf = max(r.mxf, wp[q].mxf);
      r.flags |= wp[q].flags;
    }
    part[blockIdx.x] = r;
  }
}

// new_off[f] = first kept point of frame slot >= f (the kept frame slots ascend), new_off[F] =
// kept count: one binary search per frame slot
// new_off[f] = first kept point of frame >= f: ONE WAVE per frame, a 64-ary search (64 probes
// per round: ~5 dependent rounds over 45 M points instead of a thread's 26-step binary search)
__global__ void k_land_new_off(const int32_t* __restrict__ n_kept_dev,
                               const int32_t* __restrict__ pfo, int n_frames,
                               int64_t* __restrict__ new_off) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  if (f > n_frames) return;  // (wave-uniform)
  const int64_t nk = *n_kept_dev;
  int64_t lo = 0, hi = nk;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t idx = lo + (int64_t)lane * step;
    const bool below = idx < hi && pfo[idx < hi ? idx : lo] < f;  // a prefix of the lanes
    const int c = __popcll(__ballot(below));
    if (c == 0) {
      hi = lo;
    } else {
      const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
      hi = min(hi, lo + (int64_t)c * step);
      lo = nlo;
    }
  }
  if (lane == 0) new_off[f] = (f == n_frames) ? nk : lo;
}

// The same new_off without the kept points' frame slots: k_land_compact writes a tile's kept
// points in index order, so new_off[f] = tile_base[T] + (kept points of tile T below index
// fo[f]), T = fo[f] / kCompTile (new_off_split, frame_index.h); tile_base[tile count] is the kept
// count.  One block per frame over at most one tile of cells, a thread's cells and then their
// land flags loaded together like k_land_tile_counts' (one wave per frame walking the cells 64
// at a time, two dependent loads per step, took 37 us at 1000 frames against the searched
// form's 8).
template <class CT>
__global__ __launch_bounds__(kCompBlock) void k_land_new_off_tiles(
    const int32_t* __restrict__ tile_base, const CT* __restrict__ cell,
    const uint8_t* __restrict__ land, const int64_t* __restrict__ fo,
    int64_t* __restrict__ new_off) {
  const int f = blockIdx.x;  // 0 .. n_frames
  int64_t T;
  int32_t r;
  new_off_split(fo[f], kCompTile, &T, &r);
  const int64_t b = T * kCompTile;  // b + r = fo[f] <= n: every index below b + r is a point
  int32_t cl[kCompItems];
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) {
    const int j = k * kCompBlock + (int)threadIdx.x;
    cl[k] = (j < r) ? (int32_t)cell[b + j] : -1;
  }
  uint32_t lnd[kCompItems];
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) lnd[k] = land[cl[k] >= 0 ? cl[k] : 0];
  int c = 0;
#pragma unroll
  for (int k = 0; k < kCompItems; ++k) c += (cl[k] >= 0 && !lnd[k]) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  __shared__ int ws[kCompBlock / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x / 64] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kCompBlock / 64; ++w) t += ws[w];
    new_off[f] = (int64_t)tile_base[T] + t;
  }
}

// the tiles' partials -> Bounds (what k_bounds<2> gives for the kept points with t = frame
// slot: z = 0, every t finite and integral below 2^24)
// (one 1024-thread block, four partials per thread per round with their loads issued together:
// the 12 k tile partials of a 1000-frame stack were 49 dependent rounds for 256 threads)
constexpr int kFinBlock = 1024;
__global__ __launch_bounds__(kFinBlock) void k_land_compact_final(
    const BoundsPart* __restrict__ part, int nt, const int32_t* __restrict__ n_kept_dev,
    Bounds* __restrict__ out, int64_t t_base) {
  const int64_t nk = *n_kept_dev;
  uint32_t mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u;
  int mnf = INT_MAX, mxf = INT_MIN, flags = 0;
  for (int b0 = threadIdx.x; b0 < nt; b0 += 4 * blockDim.x) {
    BoundsPart q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = part[min(b0 + u * (int)blockDim.x, nt - 1)];  // repeats
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const BoundsPart& p = q[u];
      mnx = min(mnx, p.mnx);
      mxx = max(mxx, p.mxx);
      mny = min(mny, p.mny);
      mxy = max(mxy, p.mxy);
      mnf = min(mnf, p.mnf);
      mxf = max(mxf, p.mxf);
      flags |= p.flags;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mnx = min(mnx, (uint32_t)__shfl_xor((int)mnx, off));
    mxx = max(mxx, (uint32_t)__shfl_xor((int)mxx, off));
    mny = min(mny, (uint32_t)__shfl_xor((int)mny, off));
    mxy = max(mxy, (uint32_t)__shfl_xor((int)mxy, off));
    mnf = min(mnf, __shfl_xor(mnf, off));
    mxf = max(mxf, __shfl_xor(mxf, off));
    flags |= __shfl_xor(flags, off);
  }
  __shared__ BoundsPart wp[kFinBlock / 64];
  if ((threadIdx.x & 63) == 0) wp[threadIdx.x / 64] = BoundsPart{mnx, mxx, mny, mxy, mnf, mxf, flags, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    BoundsPart r = wp[0];
    for (int q = 1; q < kFinBlock / 64; ++q) {
      r.mnx = min(r.mnx, wp[q].mnx);
      r.mxx = max(r.mxx, wp[q].mxx);
      r.mny = min(r.mny, wp[q].mny);
      r.mxy = max(r.mxy, wp[q].mxy);
      r.mnf = min(r.mnf, wp[q].mnf);
      r.mxf = max(r.mxf, wp[q].mxf);
      r.flags |= wp[q].flags;
    }
    Bounds b;
    const uint32_t z = f2ord(0.f);
    const bool any = nk > 0;
    b.mn[0] = r.mnx;
    b.mx[0] = r.mxx;
    b.mn[1] = r.mny;
    b.mx[1] = r.mxy;
    b.mn[2] = any ? z : 0xffffffffu;
    b.mx[2] = any ? z : 0u;
    const int64_t t0 = t_base + r.mnf, t1 = t_base + r.mxf;
    b.mn[3] = any ? f2ord((float)t0) : 0xffffffffu;
    b.mx[3] = any ? f2ord((float)t1) : 0u;
    b.nonfinite_xyz = (r.flags & 1) ? 1 : 0;
    b.nonintegral_t = (any && (t1 >= 16777216 || t0 <= -16777216)) ? 1 : 0;
    b.n_finite_t = (int32_t)nk;
    b.t_descends = (r.flags & 2) ? 1 : 0;
    *out = b;
  }
}
