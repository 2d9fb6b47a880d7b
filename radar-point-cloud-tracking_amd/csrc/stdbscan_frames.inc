// ST-DBSCAN, the denoise variant's kernels: launched by DbscanState::frames_pass (the min_frames
// core condition, between core_pass and union_pass) and labels_fifo (the FIFO border labels).
// frames_pass reads the sorted points, skey, the cell records, occ / occ_bits and slab_t, keeps
// its per-cell result in fok and its point queue in nc_list, and demotes core flags; labels_fifo
// reads ccmin, rep, sorig and the inverse permutation (slab) and writes the caller's labels.
//   frames_pass: k_frames_cells, k_frames_queue, k_frames_points / k_frames_points_list
//   labels_fifo: k_inverse_perm, k_label_core_orig, k_label_fifo

// ---------------------------------------------------------------- denoise variant (O8)
// PointCloudWorkF/stdbscan_denoising_pipeline.py:264-369.  A point is core when it has
// >= min_samples space-time neighbours (itself included, as K5) AND those neighbours span
// >= min_frames distinct int32(t) frames (:308-315); clusters are expanded with a FIFO queue that
// never re-queues a visited point (:346-363).  The component structure is K6's; only the core
// condition and the border rule differ (see k_label_fifo).
//
// Frames, cell level (every finite t integral: a slab is one frame): a cell whose column (same
// x, y) holds, in >= min_frames - 1 other slabs, a cell every point of which is a neighbour of
// every point of this cell (box test) has all its core points frame-complete.
__global__ __launch_bounds__(kBlock) void k_frames_cells(Geom g, int R,
                                                        const int32_t* __restrict__ occ,
                                                        const int32_t* __restrict__ n_occ,
                                                        const CellRec<2>* __restrict__ crec,
                                                        const uint32_t* __restrict__ occ_bits,
                                                        int min_frames,
                                                        uint8_t* __restrict__ fok) {
  const int64_t no = *n_occ;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < no;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t ca = occ[q];
    if ((int64_t)ca >= g.cells) continue;  // non-finite time: settled per point
    int cx, cy, cz_, cs;
    g.split((uint32_t)ca, cx, cy, cz_, cs);
    const CellRec<2> ra = crec[ca];
    const float4 A1 = rec_boxA<2>(ra), B1 = rec_boxB(ra);
    int frames = 1;  // the cell's own
    const int s0 = max(cs - R, 0), s1 = min(cs + R, g.nt - 1);
    for (int sl = s0; sl <= s1 && frames < min_frames; ++sl) {
      if (sl == cs) continue;
      const int64_t c = ((int64_t)sl * g.ny + cy) * g.nx + cx;
      if (!((occ_bits[c >> 5] >> (c & 31)) & 1u)) continue;
      const CellRec<2> rc = crec[c];
      // (box A of both cells, then box B of both: classify_cells' argument order)
      frames += (classify_cells<2>(A1, rec_boxA<2>(rc), B1, rec_boxB(rc), g) == 1) ? 1 : 0;
    }
    fok[ca] = frames >= min_frames ? 1 : 0;
  }
}

// Queue of the core points whose frame count is still open; points of the isolated cell
// (non-finite t: no neighbour, 0 frames) are settled here.
__global__ __launch_bounds__(kBlock) void k_frames_queue(const int32_t* __restrict__ skey,
                                                        int64_t n, int64_t cells,
                                                        const uint8_t* __restrict__ fok,
                                                        int min_frames, int refine,
                                                        uint8_t* __restrict__ core,
                                                        int32_t* __restrict__ list,
                                                        int32_t* __restrict__ count) {
  for (int64_t tile = (int64_t)blockIdx.x * kBlock * kItems; tile < n;
       tile += (int64_t)gridDim.x * kBlock * kItems)
    block_append(
        tile, n,
        [&](int64_t s) -> bool {
          if (!core[s]) return false;
          const int32_t key = skey[s];
          if ((int64_t)key >= cells) {
            core[s] = (min_frames <= 0) ? 1 : 0;
            return false;
          }
          return refine && !(fok && fok[key]);
        },
        list, count);
}

// Frame count of one queued core point per wave: the int32(t) offsets (within +-31 of its own:
// |dt| <= eps_t <= 30, checked by the host) of its neighbours as a 64-bit set, scanned cell by
// cell until min_frames distinct frames are seen.
template <int D>
__global__ __launch_bounds__(kBlock) void k_frames_points(const float4* __restrict__ pts,
                                                         const int32_t* __restrict__ skey, Geom g,
                                                         const CellRec<D>* __restrict__ crec,
                                                         const uint32_t* __restrict__ occ_bits,
                                                         const float2* __restrict__ slab_t,
                                                         int integral, int min_frames,
                                                         const int32_t* __restrict__ list,
                                                         const int32_t* __restrict__ count,
                                                         uint8_t* __restrict__ core) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  const int64_t nq = *count;
  for (int64_t q = w0; q < nq; q += nw) {
    const int s = list[q];
    const float4 p = pts[s];
    const int own = (int)p.w;  // numpy astype(int32): truncation toward zero
    int cx, cy, cz;
    decode_key<D>(skey[s], g, cx, cy, cz);
    const Window w = make_window<D, false>(cx, cy, cz, p.w, p.w, g, slab_t);
    uint64_t seen = 0;
    for (int base = 0; base < w.total && __popcll(seen) < min_frames; base += 64) {
      const int qq = base + lane;
      const int64_t c = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
      int b = 0, e = 0, cls = 0;
      if (c >= 0 && ((occ_bits[c >> 5] >> (c & 31)) & 1u)) {
        const CellRec<D> cr = crec[c];
        b = cr.b;
        e = cr.e;
        cls = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
      }
      uint64_t pm = __ballot(cls != 0);
      while (pm && __popcll(seen) < min_frames) {
        const int l = __ffsll((unsigned long long)pm) - 1;
        pm &= pm - 1;
        const int bb = __shfl(b, l), cl = __shfl(cls, l);
        // a whole-cell hit in frame-id data is one frame: its first point says which
        const int ee = (cl == 1 && integral) ? bb + 1 : __shfl(e, l);
        for (int j0 = bb; j0 < ee && __popcll(seen) < min_frames; j0 += 64) {
          const int j = j0 + lane;
          uint64_t bit = 0;
          if (j < ee) {
            const float4 pj = pts[j];
            if (cl == 1 || adjacent<D>(p, pj, g))  // |t| >= 2^31 (saturating casts): clamped
              bit = 1ull << min(max((int)pj.w - own + 32, 0), 63);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1)
            bit |= (uint64_t)__shfl_xor((unsigned long long)bit, off);
          seen |= bit;
        }
      }
    }
    if (lane == 0) core[s] = (__popcll(seen) >= min_frames) ? 1 : 0;
  }
}

// numpy float32 -> int32 astype on x86-64: truncation; NaN / out of range -> INT32_MIN
__device__ __forceinline__ int32_t np_i32(float v) {
  if (!(v == v) || v >= 2147483648.f || v < -2147483648.f) return INT32_MIN;
  return (int32_t)v;
}

// The same frame count for any eps_t (k_frames_points' 64-bit offset set needs |dt| <= 30): the
// distinct int32(t) frames seen so far are a list spread over the wave, kFramesPerLane per lane
// (lane k holds entries k, k + 64, ...), appended one new frame at a time, so at most
// min_frames <= 64 * kFramesPerLane entries ever exist (the host checks the bound).
constexpr int kFramesPerLane = 4;
template <int D>
__global__ __launch_bounds__(kBlock) void k_frames_points_list(
    const float4* __restrict__ pts, const int32_t* __restrict__ skey, Geom g,
    const CellRec<D>* __restrict__ crec, const uint32_t* __restrict__ occ_bits,
    const float2* __restrict__ slab_t, int integral, int min_frames,
    const int32_t* __restrict__ list, const int32_t* __restrict__ count,
    uint8_t* __restrict__ core) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  const int64_t nq = *count;
  for (int64_t q = w0; q < nq; q += nw) {
    const int s = list[q];
    const float4 p = pts[s];
    int cx, cy, cz;
    decode_key<D>(skey[s], g, cx, cy, cz);
    const Window w = make_window<D, false>(cx, cy, cz, p.w, p.w, g, slab_t);
    int32_t fr[kFramesPerLane];
#pragma unroll
    for (int k = 0; k < kFramesPerLane; ++k) fr[k] = 0;
    int nseen = 0;
    // v (this lane's candidate frame, valid when has): add it unless already listed
    auto add = [&](bool has, int32_t v) {
      bool fresh = has;
      // membership: compare against every listed entry (broadcast one register row at a time;
      // nseen is wave-uniform, so every lane runs every shuffle)
#pragma unroll
      for (int r = 0; r < kFramesPerLane; ++r) {
        if (r * 64 >= nseen) break;
        const int lim = min(nseen - r * 64, 64);
        for (int k = 0; k < lim; ++k) {
          const int32_t e = __shfl(fr[r], k);
          if (e == v) fresh = false;
        }
      }
      // append the distinct fresh values, lowest lane first
      uint64_t m = __ballot(fresh);
      while (m && nseen < min_frames) {
        const int l = __ffsll((unsigned long long)m) - 1;
        const int32_t nv = __shfl(v, l);
        const int r = nseen / 64, k = nseen % 64;
#pragma unroll
        for (int rr = 0; rr < kFramesPerLane; ++rr)
          if (rr == r && lane == k) fr[rr] = nv;
        ++nseen;
        if (fresh && v == nv) fresh = false;
        m = __ballot(fresh);
      }
    };
    for (int base = 0; base < w.total && nseen < min_frames; base += 64) {
      const int qq = base + lane;
      const int64_t c = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
      int b = 0, e = 0, cls = 0;
      if (c >= 0 && ((occ_bits[c >> 5] >> (c & 31)) & 1u)) {
        const CellRec<D> cr = crec[c];
        b = cr.b;
        e = cr.e;
        cls = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
      }
      uint64_t pm = __ballot(cls != 0);
      while (pm && nseen < min_frames) {
        const int l = __ffsll((unsigned long long)pm) - 1;
        pm &= pm - 1;
        const int bb = __shfl(b, l), cl = __shfl(cls, l);
        // a whole-cell hit in frame-id data is one frame: its first point says which
        const int ee = (cl == 1 && integral) ? bb + 1 : __shfl(e, l);
        for (int j0 = bb; j0 < ee && nseen < min_frames; j0 += 64) {
          const int j = j0 + lane;
          bool has = false;
          int32_t v = 0;
          if (j < ee) {
            const float4 pj = pts[j];
            if (cl == 1 || adjacent<D>(p, pj, g)) {
              has = true;
              v = np_i32(pj.w);
            }
          }
          add(has, v);
        }
      }
    }
    if (lane == 0) core[s] = (nseen >= min_frames) ? 1 : 0;
  }
}

// spos[orig] = sorted position (when the grid build did not write it)
__global__ void k_inverse_perm(const int32_t* __restrict__ sorig, int64_t n,
                               int32_t* __restrict__ spos) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    spos[sorig[s]] = (int32_t)s;
}

// Border labels of the FIFO expansion (:340-367).  Clusters are drained one after another in
// seed order, the seed being the component's minimum core index m (what ccmin holds).  A non-core
// point p (original index P) is popped by cluster m -- and keeps the first such label -- iff it is
// adjacent to a core point of m and either P > m (still unvisited when m's cores expand) or p is a
// neighbour of the seed itself (the seed's neighbour list is queued whole, visited or not, :343).
// Every qualifying m < P beats every m > P, so the first kind is a plain minimum and the second is
// resolved smallest-first with one seed test per distinct m.  One wave per non-core point.
template <int D>
__global__ __launch_bounds__(kBlock) void k_label_fifo(const float4* __restrict__ pts,
                                                      const int32_t* __restrict__ skey, Geom g,
                                                      const CellRec<D>* __restrict__ crec,
                                                      const uint32_t* __restrict__ occ_bits,
                                                      const float2* __restrict__ slab_t,
                                                      const int32_t* __restrict__ ccmin,
                                                      const int32_t* __restrict__ rep,
                                                      const int32_t* __restrict__ sorig,
                                                      const int32_t* __restrict__ spos,
                                                      MinRank cid,
                                                      const int32_t* __restrict__ nc_list,
                                                      const int32_t* __restrict__ nc_count,
                                                      int32_t* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  const int64_t nq = *nc_count;
  for (int64_t q = w0; q < nq; q += nw) {
    const int s = nc_list[q];
    const int P = sorig[s];
    const int32_t key = skey[s];
    int best_lt = INT_MAX, best_gt = INT_MAX;
    if ((int64_t)key < g.cells) {
      const float4 p = pts[s];
      int cx, cy, cz;
      decode_key<D>(key, g, cx, cy, cz);
      const Window w = make_window<D, false>(cx, cy, cz, p.w, p.w, g, slab_t);
      for (int base = 0; base < w.total; base += 64) {
        const int qq = base + lane;
        const int64_t c = (qq < w.total) ? window_cell<D>(w, qq, g, slab_t, p.w, p.w) : -1;
        int b = 0, e = 0, cls = 0;
        if (c >= 0 && ((occ_bits[c >> 5] >> (c & 31)) & 1u) && rep[c] >= 0) {
          const CellRec<D> cr = crec[c];
          b = cr.b;
          e = cr.e;
          cls = classify<D>(p, rec_boxA<D>(cr), rec_boxB(cr), g);
        }
        uint64_t pm = __ballot(cls != 0);
        while (pm) {
          const int l = __ffsll((unsigned long long)pm) - 1;
          pm &= pm - 1;
          const int bb = __shfl(b, l), ee = __shfl(e, l), cl = __shfl(cls, l);
          for (int j0 = bb; j0 < ee; j0 += 64) {
            const int j = j0 + lane;
            int m = -1;
            if (j < ee) {
              m = ccmin[j];
              if (m >= 0 && cl != 1 && !adjacent<D>(p, pts[j], g)) m = -1;
            }
            int lt = (m >= 0 && m < P) ? m : INT_MAX;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) lt = min(lt, __shfl_xor(lt, off));
            best_lt = min(best_lt, lt);
            if (best_lt != INT_MAX) continue;  // a smaller qualifying cluster is known
            // m > P: the smallest not yet rejected whose seed is a neighbour of p
            int cand = (m > P && m < best_gt) ? m : INT_MAX;
            while (true) {
              int mm = cand;
#pragma unroll
              for (int off = 32; off > 0; off >>= 1) mm = min(mm, __shfl_xor(mm, off));
              if (mm == INT_MAX) break;
              if (adjacent<D>(p, pts[spos[mm]], g)) {
                best_gt = mm;
                break;
              }
              if (cand == mm) cand = INT_MAX;
            }
          }
        }
      }
    }
    if (lane == 0) {
      const int best = (best_lt != INT_MAX) ? best_lt : best_gt;
      labels[P] = (best != INT_MAX) ? cid[best] : -1;
    }
  }
}
