// ST-DBSCAN stage K4, the grid build: launched by DbscanState::build_t.  Reads
// stdbscan_shared.inc only.
// Reads the caller's x, y, (z,) t.  Leaves behind the sorted points (pts: float4 {x, y, z|t, t},
// or float2 {x, y} where DbscanState::xy_points) with sorig (original index) and skey (cell key)
// per sorted point, and the inverse permutation in slab where spos_on; cell_start[C + 1]; the
// occupied cells, ascending, in occ (their count on the device at n_occ_dev) and as occ_bits; the
// cell records crec with mutual; slab_t; and, where the fused K5 takes them from here, the
// all-core cells' minima in cell_min_pair.  hpos, the radix key buffers (the chunk histograms),
// cell_min and cell_root (the coalesced scan's flags) are scratch of the build.
//   k_bounds, k_bounds_final   min/max per dimension and time, "times integral" flag (1 sync)
//   time-ordered finite 2-D points, a slab's cells within LDS: a counting sort per slab
//     k_slab_lo, then k_slab_bucket (one block per slab), or in chunks k_slab_chunk_hist,
//     k_slab_chunk_scan (or k_chunk_totals, k_chunk_cursors, k_occ_write, k_cell_start_end,
//     k_slab_occ_base around two scans) and k_slab_chunk_scatter; a scan and k_occ_gather
//     (the writers: sorted float4 {x, y, t, t}, or float2 {x, y} where no kernel of the run
//     needs a point's time, DbscanState::xy_points)
//   otherwise k_keys (cell key per point: ((slab*nz + cz)*ny + cy)*nx + cx), a stable radix
//     sort, k_gather (sorted float4 {x, y, z|t, t} + original index), k_cell_runs, scans ->
//     cell_start[C+1], k_occ_list
//   k_cell_box / k_cell_box_mixed   per occupied cell: point range, bounding box in space and
//     time, "mutual" flag (box diagonal within eps and time span within eps_t: every pair
//     adjacent); k_slab_range: the time range per slab

template <int D>
__global__ __launch_bounds__(kBlock) void k_bounds(const float* __restrict__ x,
                                                  const float* __restrict__ y,
                                                  const float* __restrict__ z, int64_t stride,
                                                  const float* __restrict__ t, int64_t n,
                                                  Bounds* __restrict__ out,
                                                  const int64_t* __restrict__ n_dev = nullptr) {
  if (n_dev) n = *n_dev;  // count on the device (at most the host n the grid was sized for)
  uint32_t mn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  uint32_t mx[4] = {0u, 0u, 0u, 0u};
  int nonfin = 0, nonint = 0, nfin = 0, desc = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v[4];
    v[0] = x[i * stride];
    v[1] = y[i * stride];
    v[2] = (D == 3) ? z[i * stride] : 0.f;
    v[3] = t[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!isfinite(v[k])) nonfin = 1;
      uint32_t o = f2ord(v[k]);
      mn[k] = min(mn[k], o);
      mx[k] = max(mx[k], o);
    }
    if (isfinite(v[3])) {
      ++nfin;
      uint32_t o = f2ord(v[3]);
      mn[3] = min(mn[3], o);
      mx[3] = max(mx[3], o);
      if (v[3] != floorf(v[3]) || fabsf(v[3]) >= 16777216.f) nonint = 1;
    }
    if (i > 0 && !(t[i - 1] <= v[3])) desc = 1;  // NaN counts as out of order
  }
  // wave reduce, then one partial per block
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], off));
      mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], off));
    }
    nonfin |= __shfl_xor(nonfin, off);
    nonint |= __shfl_xor(nonint, off);
    nfin += __shfl_xor(nfin, off);
    desc |= __shfl_xor(desc, off);
  }
  __shared__ uint32_t smn[kBlock / 64][4], smx[kBlock / 64][4];
  __shared__ int sfl[kBlock / 64][4];
  const int w = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 4; ++k) {
      smn[w][k] = mn[k];
      smx[w][k] = mx[k];
    }
    sfl[w][0] = nonfin;
    sfl[w][1] = nonint;
    sfl[w][2] = nfin;
    sfl[w][3] = desc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kBlock / 64; ++v) {
      for (int k = 0; k < 4; ++k) {
        mn[k] = min(mn[k], smn[v][k]);
        mx[k] = max(mx[k], smx[v][k]);
      }
      nonfin |= sfl[v][0];
      nonint |= sfl[v][1];
      nfin += sfl[v][2];
      desc |= sfl[v][3];
    }
    // per-block partial, reduced by k_bounds_final (no same-address atomics)
    Bounds& o = out[blockIdx.x];
    for (int k = 0; k < 4; ++k) {
      o.mn[k] = mn[k];
      o.mx[k] = mx[k];
    }
    o.nonfinite_xyz = nonfin;
    o.nonintegral_t = nonint;
    o.n_finite_t = nfin;
    o.t_descends = desc;
  }
}

__global__ __launch_bounds__(kBlock) void k_bounds_final(const Bounds* __restrict__ part, int nb,
                                                        Bounds* __restrict__ out) {
  uint32_t mn[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  uint32_t mx[4] = {0u, 0u, 0u, 0u};
  int nonfin = 0, nonint = 0, nfin = 0, desc = 0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    const Bounds& p = part[b];
    for (int k = 0; k < 4; ++k) {
      mn[k] = min(mn[k], p.mn[k]);
      mx[k] = max(mx[k], p.mx[k]);
    }
    nonfin |= p.nonfinite_xyz;
    nonint |= p.nonintegral_t;
    nfin += p.n_finite_t;
    desc |= p.t_descends;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], off));
      mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], off));
    }
    nonfin |= __shfl_xor(nonfin, off);
    nonint |= __shfl_xor(nonint, off);
    nfin += __shfl_xor(nfin, off);
    desc |= __shfl_xor(desc, off);
  }
  __shared__ Bounds sb[kBlock / 64];
  const int w = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 4; ++k) {
      sb[w].mn[k] = mn[k];
      sb[w].mx[k] = mx[k];
    }
    sb[w].nonfinite_xyz = nonfin;
    sb[w].nonintegral_t = nonint;
    sb[w].n_finite_t = nfin;
    sb[w].t_descends = desc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < kBlock / 64; ++v) {
      for (int k = 0; k < 4; ++k) {
        mn[k] = min(mn[k], sb[v].mn[k]);
        mx[k] = max(mx[k], sb[v].mx[k]);
      }
      nonfin |= sb[v].nonfinite_xyz;
      nonint |= sb[v].nonintegral_t;
      nfin += sb[v].n_finite_t;
      desc |= sb[v].t_descends;
    }
    for (int k = 0; k < 4; ++k) {
      out->mn[k] = mn[k];
      out->mx[k] = mx[k];
    }
    out->nonfinite_xyz = nonfin;
    out->nonintegral_t = nonint;
    out->n_finite_t = nfin;
    out->t_descends = desc;
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_keys(const float* __restrict__ x,
                                                const float* __restrict__ y,
                                                const float* __restrict__ z, int64_t stride,
                                                const float* __restrict__ t, int64_t n, Geom g,
                                                uint32_t* __restrict__ keys,
                                                uint32_t* __restrict__ vals) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float ti = t[i];
    uint32_t key;
    if (!isfinite(ti)) {
      key = (uint32_t)g.cells;  // isolated: matches nothing, not even itself
    } else {
      const int cx = cell_of((double)x[i * stride], g.ox, g.inv_cs, g.nx);
      const int cy = cell_of((double)y[i * stride], g.oy, g.inv_cs, g.ny);
      const int cz = (D == 3) ? cell_of((double)z[i * stride], g.oz, g.inv_cs, g.nz) : 0;
      const int s = slab_of(ti, g);
      key = (uint32_t)((((int64_t)s * g.nz + cz) * g.ny + cy) * g.nx + cx);
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_gather(const float* __restrict__ x,
                                                  const float* __restrict__ y,
                                                  const float* __restrict__ z, int64_t stride,
                                                  const float* __restrict__ t, int64_t n,
                                                  const uint32_t* __restrict__ skeys,
                                                  const uint32_t* __restrict__ svals,
                                                  float4* __restrict__ pts,
                                                  int32_t* __restrict__ sorig,
                                                  int32_t* __restrict__ skey,
                                                  int32_t* __restrict__ spos) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = svals[s];
    float4 p;
    p.x = x[i * stride];
    p.y = y[i * stride];
    p.w = t[i];
    p.z = (D == 3) ? z[i * stride] : p.w;
    pts[s] = p;
    sorig[s] = (int32_t)i;
    if (spos) spos[i] = (int32_t)s;
    skey[s] = (int32_t)skeys[s];
  }
}

// Cell occupancy from the sorted keys (no atomics on hot cells): a run's head subtracts its start
// and its tail adds its end, so cell_count[c] = run length (two uncontended atomics per occupied
// cell); head flags (scanned later) give the occupied-cell list in ascending key order.
__global__ __launch_bounds__(kBlock) void k_cell_runs(const int32_t* __restrict__ skey, int64_t n,
                                                     int32_t* __restrict__ cell_count,
                                                     int32_t* __restrict__ head) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = skey[s];
    const bool h = (s == 0) || skey[s - 1] != k;
    const bool t = (s == n - 1) || skey[s + 1] != k;
    if (h && t) {
      cell_count[k] = 1;
    } else {
      if (h) atomicAdd(cell_count + k, -(int32_t)s);
      if (t) atomicAdd(cell_count + k, (int32_t)(s + 1));
    }
    head[s] = h ? 1 : 0;
  }
}

// pos = exclusive scan of the head flags: cell of every run head -> occ[pos]
// (+ the occupancy bitmap: one bit per cell, small enough to stay in L2, so window scans skip
// empty candidate cells without reading their records)
__global__ __launch_bounds__(kBlock) void k_occ_list(const int32_t* __restrict__ skey, int64_t n,
                                                    const int32_t* __restrict__ pos,
                                                    int32_t* __restrict__ occ,
                                                    uint32_t* __restrict__ occ_bits) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    if (pos[s + 1] != pos[s]) {
      const int32_t c = skey[s];
      occ[pos[s]] = c;
      atomicOr(occ_bits + (c >> 5), 1u << (c & 31));
    }
}

// ---- K4 for time-ordered 2-D input (the stack path: points come frame-major from K1 / the land
// filter, and a slab is a frame): the cell sort is a counting sort of each slab's points by their
// (y, x) cell, one 1024-thread block per slab with the slab's cell histogram in LDS.  It replaces
// keys + three radix passes + the gather + the cell-count pass: two reads of x / y (/ t) and one
// scattered write of the sorted records per point, and the dense cell_start rows come out of the
// histogram scan directly.  Order inside a cell is arrival order: nothing downstream depends on
// it (roots are minimum ORIGINAL indices, counts and minima are order-free).
constexpr int kBucketBlock = 1024;
constexpr int kBucketCells = 16384;  // max per-slab cells for the LDS histogram (<= 64 KiB)
constexpr int kBucketU = 4;          // points per thread per round (loads in flight together)
constexpr int64_t kChunkPts = 16384;  // points per slab-bucket block when a slab is split

// occ_base[s] = the first occupied-list position of slab s (the flags' exclusive scan at the
// slab's first cell), occ_base[nt] = the occupied count
__global__ void k_slab_occ_base(const int32_t* __restrict__ pos, int P, int64_t nt,
                                int32_t* __restrict__ occ_base) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= nt;
       s += (int64_t)gridDim.x * blockDim.x)
    occ_base[s] = pos[s * P];
}

// cell_start[cells] = n (the scan's total) -> the isolated cell (empty) ends there too
__global__ void k_cell_start_end(int32_t* __restrict__ cell_start, int64_t cells) {
  if (threadIdx.x == 0) cell_start[cells + 1] = cell_start[cells];
}

// slab_lo[s] = first point of slab s (points ordered by slab), slab_lo[nt] = n: ONE WAVE per
// slab, a 64-ary search (64 probes per round: ~5 dependent rounds over 50 M points instead of a
// thread's 26-step binary search).  Also clears zero[0, zwords) (the occupancy bits the slab
// bucket sets next: one launch instead of a memset and this).
__global__ void k_slab_lo(const float* __restrict__ t, int64_t n, Geom g,
                          int32_t* __restrict__ slab_lo, uint32_t* __restrict__ zero,
                          int64_t zwords) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < zwords;
       i += (int64_t)gridDim.x * blockDim.x)
    zero[i] = 0u;
  const int lane = threadIdx.x & 63;
  const int64_t wpb = blockDim.x / 64;
  for (int64_t s = (int64_t)blockIdx.x * wpb + threadIdx.x / 64; s <= g.nt;
       s += (int64_t)gridDim.x * wpb) {
    int64_t lo = 0, hi = n;  // the first point of slab >= s lies in [lo, hi]
    while (lo < hi) {
      const int64_t step = (hi - lo + 63) / 64;
      const int64_t idx = lo + (int64_t)lane * step;
      const bool below = idx < hi && slab_of(t[idx < hi ? idx : lo], g) < s;  // a lane prefix
      const int c = __popcll(__ballot(below));
      if (c == 0) {
        hi = lo;
      } else {
        const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
        hi = min(hi, lo + (int64_t)c * step);
        lo = nlo;
      }
    }
    if (lane == 0) slab_lo[s] = (int32_t)(s == g.nt ? n : lo);
  }
}

// XY: float2 points, no per-point time load; slab_t[s] written here (see slab_time_of)
template <bool XY>
__global__ __launch_bounds__(kBucketBlock) void k_slab_bucket(
    const float* __restrict__ x, const float* __restrict__ y, int64_t stride,
    const float* __restrict__ t, Geom g, const int32_t* __restrict__ slab_lo,
    Pt<XY>* __restrict__ pts, int32_t* __restrict__ sorig, int32_t* __restrict__ skey,
    int32_t* __restrict__ spos, int32_t* __restrict__ cell_start, int32_t* __restrict__ occ_tmp,
    int32_t* __restrict__ slab_occ, uint32_t* __restrict__ occ_bits,
    unsigned long long* __restrict__ cmin_all, float2* __restrict__ slab_t) {
  // the slab's nx * ny cell counts, sized at launch (a 463-m sweep at cells of 5.6 m: 27 KiB, so
  // several slabs share a CU instead of one 64-KiB histogram each)
  // cmin_all (nullable; the fused K5): every occupied cell's (min original, sorted) pair over all
  // its points -- the smallest index per cell by an LDS atomicMin per run in the count pass (a
  // run's head lane holds its smallest index), written by that point at its scatter
  extern __shared__ int32_t hist[];
  __shared__ int32_t wsum[kBucketBlock / 64], wocc[kBucketBlock / 64];
  const int s = blockIdx.x;
  const int P = g.nx * g.ny;
  int32_t* mn = hist + P;  // (cmin_all only: the launch sizes 2P words)
  const int lo = slab_lo[s], hi = slab_lo[s + 1];
  if (XY && threadIdx.x == 0) slab_t[s] = slab_time_of(t, lo, hi);
  for (int c = threadIdx.x; c < P; c += kBucketBlock) {
    hist[c] = 0;
    if (cmin_all) mn[c] = INT_MAX;
  }
  __syncthreads();
  // consecutive points (along a ray) often share a cell: a run of equal cells in a wave takes
  // ONE LDS atomic (by its head lane) instead of one per point
  const int ln = threadIdx.x & 63;
  auto runs = [&](int c, bool v, int& rank, int& len, int& head) {
    const int up = __shfl_up(c, 1, 64), dn = __shfl_down(c, 1, 64);
    const uint64_t hm = __ballot(v && (ln == 0 || up != c));
    const uint64_t lm = __ballot(v && (ln == 63 || dn != c));
    const uint64_t below = (ln == 63) ? ~0ull : ((2ull << ln) - 1ull);
    head = 63 - __builtin_clzll((hm & below) | 1ull);  // hm has a bit at or below ln when v
    const int last = ln + __builtin_ctzll((lm >> ln) | (1ull << (63 - ln)));
    rank = ln - head;
    len = last - head + 1;
  };
  // kBucketU points per thread per round, their loads issued together
  auto cell_xy = [&](float px, float py) {
    return cell_of((double)py, g.oy, g.inv_cs, g.ny) * g.nx +
           cell_of((double)px, g.ox, g.inv_cs, g.nx);
  };
  for (int i0 = lo; i0 < hi; i0 += kBucketBlock * kBucketU) {
    // loads from clamped indices (the slab is not empty here): a conditional load would be a
    // branch ending in a full vmcnt wait, one round trip per point instead of per round
    float px[kBucketU], py[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = min(i0 + u * kBucketBlock + (int)threadIdx.x, hi - 1);
      px[u] = x[(int64_t)i * stride];
      py[u] = y[(int64_t)i * stride];
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = i0 + u * kBucketBlock + threadIdx.x;
      const bool v = i < hi;
      const int c = v ? cell_xy(px[u], py[u]) : -1;
      int rank, len, head;
      runs(c, v, rank, len, head);
      if (v && rank == 0) {
        atomicAdd(&hist[c], len);
        if (cmin_all) atomicMin(&mn[c], i);
      }
    }
  }
  __syncthreads();
  // exclusive scan of hist[0, P): each thread a contiguous run, then the block's run sums
  const int per = (P + kBucketBlock - 1) / kBucketBlock;
  const int c0 = threadIdx.x * per, c1 = min(c0 + per, P);
  int run = 0, orun = 0;
  for (int c = c0; c < c1; ++c) {
    const int h = hist[c];
    run += h;
    orun += (h > 0) ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
  int incl = run, oincl = orun;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    const int oo = __shfl_up(oincl, off, 64);
    if (lane >= off) {
      incl += o;
      oincl += oo;
    }
  }
  if (lane == 63) {
    wsum[w] = incl;
    wocc[w] = oincl;
  }
  __syncthreads();
  int before = 0, obefore = 0, otot = 0;
  for (int v = 0; v < kBucketBlock / 64; ++v) {
    if (v < w) {
      before += wsum[v];
      obefore += wocc[v];
    }
    otot += wocc[v];
  }
  int acc = before + incl - run;
  // the slab's occupied cells, ascending, at the front of its point range (a slab has no more
  // occupied cells than points), and their occupancy bits (one atomicOr per word of this run)
  int oacc = lo + obefore + oincl - orun;
  uint32_t word = 0xffffffffu, mask = 0u;
  for (int c = c0; c < c1; ++c) {
    const int h = hist[c];
    hist[c] = acc;
    cell_start[(int64_t)s * P + c] = lo + acc;
    acc += h;
    if (h > 0) {
      const int64_t key = (int64_t)s * P + c;
      occ_tmp[oacc++] = (int32_t)key;
      const uint32_t wd = (uint32_t)(key >> 5);
      if (wd != word) {
        if (mask) atomicOr(occ_bits + word, mask);
        word = wd;
        mask = 0u;
      }
      mask |= 1u << (key & 31);
    }
  }
  if (mask) atomicOr(occ_bits + word, mask);
  if (threadIdx.x == 0) slab_occ[s] = otot;
  __syncthreads();
  for (int i0 = lo; i0 < hi; i0 += kBucketBlock * kBucketU) {
    float px[kBucketU], py[kBucketU], pt[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = min(i0 + u * kBucketBlock + (int)threadIdx.x, hi - 1);  // branch-free
      px[u] = x[(int64_t)i * stride];
      py[u] = y[(int64_t)i * stride];
      pt[u] = XY ? 0.f : t[i];
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = i0 + u * kBucketBlock + threadIdx.x;
      const bool v = i < hi;
      const int c = v ? cell_xy(px[u], py[u]) : -1;
      int rank, len, head;
      runs(c, v, rank, len, head);
      int base = (v && rank == 0) ? atomicAdd(&hist[c], len) : 0;
      base = __shfl(base, head, 64);
      if (v) {
        const int dst = lo + base + rank;
        store_pt<XY>(pts, dst, px[u], py[u], pt[u]);
        sorig[dst] = i;
        if (spos) spos[i] = dst;  // (kernel-uniform; coalesced: i runs over the lanes)
        skey[dst] = s * P + c;
        if (cmin_all && mn[c] == i)
          cmin_all[(int64_t)s * P + c] = ((unsigned long long)(uint32_t)i << 32) | (uint32_t)dst;
      }
    }
  }
  if (s == g.nt - 1 && threadIdx.x == 0) {  // the isolated cell (empty here) and the end
    cell_start[g.cells] = hi;
    cell_start[g.cells + 1] = hi;
  }
}

// Several blocks per slab (dense slabs: one block per slab leaves most CUs idle and serialises
// hundreds of thousands of points per block).  Chunk ch of slab s is its points
// [lo + ch*len/CH, lo + (ch+1)*len/CH).  hist: [nt][CH][P] per-chunk cell counts, turned by
// k_slab_chunk_scan into per-chunk write cursors; the scan also writes cell_start, the slab's
// occupied cells + bits and its occupied count exactly like k_slab_bucket.
__device__ __forceinline__ void slab_chunk(const int32_t* __restrict__ slab_lo, int s, int ch,
                                           int CH, int& lo, int& hi) {
  const int a = slab_lo[s], b = slab_lo[s + 1];
  const int64_t len = (int64_t)(b - a);
  lo = a + (int)(len * ch / CH);
  hi = a + (int)(len * (ch + 1) / CH);
}

__global__ __launch_bounds__(kBucketBlock) void k_slab_chunk_hist(
    const float* __restrict__ x, const float* __restrict__ y, int64_t stride, Geom g,
    const int32_t* __restrict__ slab_lo, int CH, int32_t* __restrict__ hist_g) {
  extern __shared__ int32_t hist[];
  const int s = blockIdx.x / CH, ch = blockIdx.x - s * CH;
  const int P = g.nx * g.ny;
  int lo, hi;
  slab_chunk(slab_lo, s, ch, CH, lo, hi);
  for (int c = threadIdx.x; c < P; c += kBucketBlock) hist[c] = 0;
  __syncthreads();
  for (int i0 = lo; i0 < hi; i0 += kBucketBlock * kBucketU) {
    float px[kBucketU], py[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = min(i0 + u * kBucketBlock + (int)threadIdx.x, hi - 1);  // branch-free
      px[u] = x[(int64_t)i * stride];
      py[u] = y[(int64_t)i * stride];
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = i0 + u * kBucketBlock + threadIdx.x;
      if (i < hi)
        atomicAdd(&hist[cell_of((double)py[u], g.oy, g.inv_cs, g.ny) * g.nx +
                        cell_of((double)px[u], g.ox, g.inv_cs, g.nx)], 1);
    }
  }
  __syncthreads();
  int32_t* out = hist_g + (int64_t)blockIdx.x * P;
  for (int c = threadIdx.x; c < P; c += kBucketBlock) out[c] = hist[c];
}

__global__ __launch_bounds__(kBucketBlock) void k_slab_chunk_scan(
    Geom g, const int32_t* __restrict__ slab_lo, int CH, int32_t* __restrict__ hist_g,
    int32_t* __restrict__ cell_start, int32_t* __restrict__ occ_tmp,
    int32_t* __restrict__ slab_occ, uint32_t* __restrict__ occ_bits) {
  __shared__ int32_t wsum[kBucketBlock / 64], wocc[kBucketBlock / 64];
  const int s = blockIdx.x;
  const int P = g.nx * g.ny;
  const int lo = slab_lo[s], hi = slab_lo[s + 1];
  int32_t* hs = hist_g + (int64_t)s * CH * P;
  const int per = (P + kBucketBlock - 1) / kBucketBlock;
  const int c0 = threadIdx.x * per, c1 = min(c0 + per, P);
  int run = 0, orun = 0;
  for (int c = c0; c < c1; ++c) {
    int h = 0;
    for (int ch = 0; ch < CH; ++ch) h += hs[(int64_t)ch * P + c];
    run += h;
    orun += (h > 0) ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
  int incl = run, oincl = orun;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    const int oo = __shfl_up(oincl, off, 64);
    if (lane >= off) {
      incl += o;
      oincl += oo;
    }
  }
  if (lane == 63) {
    wsum[w] = incl;
    wocc[w] = oincl;
  }
  __syncthreads();
  int before = 0, obefore = 0, otot = 0;
  for (int v = 0; v < kBucketBlock / 64; ++v) {
    if (v < w) {
      before += wsum[v];
      obefore += wocc[v];
    }
    otot += wocc[v];
  }
  int acc = before + incl - run;
  int oacc = lo + obefore + oincl - orun;
  uint32_t word = 0xffffffffu, mask = 0u;
  for (int c = c0; c < c1; ++c) {
    cell_start[(int64_t)s * P + c] = lo + acc;
    int h = 0;
    for (int ch = 0; ch < CH; ++ch) {  // per-chunk cursors (slab-local), chunk order
      const int k = hs[(int64_t)ch * P + c];
      hs[(int64_t)ch * P + c] = acc + h;
      h += k;
    }
    acc += h;
    if (h > 0) {
      const int64_t key = (int64_t)s * P + c;
      occ_tmp[oacc++] = (int32_t)key;
      const uint32_t wd = (uint32_t)(key >> 5);
      if (wd != word) {
        if (mask) atomicOr(occ_bits + word, mask);
        word = wd;
        mask = 0u;
      }
      mask |= 1u << (key & 31);
    }
  }
  if (mask) atomicOr(occ_bits + word, mask);
  if (threadIdx.x == 0) slab_occ[s] = otot;
  if (s == g.nt - 1 && threadIdx.x == 0) {  // the isolated cell (empty here) and the end
    cell_start[g.cells] = hi;
    cell_start[g.cells + 1] = hi;
  }
}

// The same outputs as k_slab_chunk_scan from fully parallel, coalesced passes over every
// (slab, cell) -- one block per slab walking its cells in per-thread runs left most CUs idle
// and read the [chunk][cell] histograms with a lane stride (2.2 GB per dense 125-frame share):
//   k_chunk_totals   cell_start[key] = the cell's count over the slab's chunks
//   (in-place exclusive scan of cell_start: the points are slab-major, so the global prefix IS
//    every cell's first point)
//   k_chunk_cursors  per-chunk slab-local write cursors, occupancy words (one ballot per 64
//                    keys), occupied flags
//   (exclusive scan of the flags) -> k_occ_write: the ascending occupied list and its count.
__global__ void k_chunk_totals(const int32_t* __restrict__ hist_g, int64_t cells, int P, int CH,
                               int32_t* __restrict__ cell_start) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cells;
       k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = k / P;
    const int32_t* h = hist_g + s * (int64_t)CH * P + (k - s * P);
    int t = 0;
    for (int ch = 0; ch < CH; ++ch) t += h[(int64_t)ch * P];
    cell_start[k] = t;
  }
}

__global__ void k_chunk_cursors(int32_t* __restrict__ hist_g, int64_t cells, int P, int CH,
                                const int32_t* __restrict__ cell_start,
                                const int32_t* __restrict__ slab_lo,
                                uint32_t* __restrict__ occ_bits, int32_t* __restrict__ occf) {
  // whole waves over 64 consecutive keys (the grid stride is a multiple of 64): the wave's
  // ballot of occupied cells is two whole occupancy words
  const int lane = threadIdx.x & 63;
  for (int64_t k0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~(int64_t)63; k0 < cells;
       k0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = k0 + lane;
    bool o = false;
    if (k < cells) {
      const int64_t s = k / P;
      int32_t* h = hist_g + s * (int64_t)CH * P + (k - s * P);
      int acc = cell_start[k] - slab_lo[s];
      const int first = acc;
      for (int ch = 0; ch < CH; ++ch) {
        const int v = h[(int64_t)ch * P];
        h[(int64_t)ch * P] = acc;
        acc += v;
      }
      o = acc > first;
      occf[k] = o ? 1 : 0;
    }
    const uint64_t m = __ballot(o);
    if (lane == 0) occ_bits[k0 >> 5] = (uint32_t)m;
    if (lane == 32) occ_bits[(k0 >> 5) + 1] = (uint32_t)(m >> 32);
  }
}

__global__ void k_occ_write(const int32_t* __restrict__ occf, const int32_t* __restrict__ pos,
                            int64_t cells, int32_t* __restrict__ occ) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cells;
       k += (int64_t)gridDim.x * blockDim.x)
    if (occf[k]) occ[pos[k]] = (int32_t)k;
}

// XY: as k_slab_bucket<true> (a slab's first chunk writes slab_t[s])
template <bool XY>
__global__ __launch_bounds__(kBucketBlock) void k_slab_chunk_scatter(
    const float* __restrict__ x, const float* __restrict__ y, int64_t stride,
    const float* __restrict__ t, Geom g, const int32_t* __restrict__ slab_lo, int CH,
    const int32_t* __restrict__ hist_g, Pt<XY>* __restrict__ pts, int32_t* __restrict__ sorig,
    int32_t* __restrict__ skey, int32_t* __restrict__ spos, float2* __restrict__ slab_t) {
  extern __shared__ int32_t cur[];
  const int s = blockIdx.x / CH, ch = blockIdx.x - s * CH;
  const int P = g.nx * g.ny;
  int lo, hi;
  slab_chunk(slab_lo, s, ch, CH, lo, hi);
  const int base = slab_lo[s];
  if (XY && ch == 0 && threadIdx.x == 0) slab_t[s] = slab_time_of(t, base, slab_lo[s + 1]);
  const int32_t* hc = hist_g + (int64_t)blockIdx.x * P;
  for (int c = threadIdx.x; c < P; c += kBucketBlock) cur[c] = hc[c];
  __syncthreads();
  for (int i0 = lo; i0 < hi; i0 += kBucketBlock * kBucketU) {
    float px[kBucketU], py[kBucketU], pt[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = min(i0 + u * kBucketBlock + (int)threadIdx.x, hi - 1);  // branch-free
      px[u] = x[(int64_t)i * stride];
      py[u] = y[(int64_t)i * stride];
      pt[u] = XY ? 0.f : t[i];
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int i = i0 + u * kBucketBlock + threadIdx.x;
      if (i < hi) {
        const int c = cell_of((double)py[u], g.oy, g.inv_cs, g.ny) * g.nx +
                      cell_of((double)px[u], g.ox, g.inv_cs, g.nx);
        const int dst = base + atomicAdd(&cur[c], 1);
        store_pt<XY>(pts, dst, px[u], py[u], pt[u]);
        sorig[dst] = i;
        if (spos) spos[i] = dst;  // (kernel-uniform; coalesced: i runs over the lanes)
        skey[dst] = s * P + c;
      }
    }
  }
}

// the slabs' occupied-cell runs (k_slab_bucket, at each slab's point offset) -> the ascending list
__global__ __launch_bounds__(kBlock) void k_occ_gather(const int32_t* __restrict__ occ_tmp,
                                                      const int32_t* __restrict__ slab_lo,
                                                      const int32_t* __restrict__ occ_base,
                                                      int32_t* __restrict__ occ) {
  const int s = blockIdx.x;
  const int b = occ_base[s], m = occ_base[s + 1] - b, lo = slab_lo[s];
  for (int j = threadIdx.x; j < m; j += blockDim.x) occ[b + j] = occ_tmp[lo + j];
}

// Per-cell records (point range and bounding box in space and time; the only copy of the boxes:
// the per-point union reads them from the records too), kCbLanes lanes per occupied cell, four
// cells per wave.  A wave waits for its densest cell (a few hundred points at the standard
// density, thousands in the dense stacks), so lanes per cell set the rate: same-box A/B
// (tools/kab2.sh, 1000 standard / 125 dense frames) 4 lanes 434 / 403 us, 8 lanes 353 / 347,
// 16 lanes 347 / 321, 32 lanes 453 / 387.  mutual[c] = 1 when every pair of points in the cell
// passes the neighbour test (computed conservatively from the box with the same rounding as the
// pair test).
// XY (2-D, float2 points): the time fields come from the slab's one time value (slab_t, filled by
// the grid build's writer), not from a reduction over equal values.
constexpr int kCbLanes = 16;
template <int D, bool XY = false>
__global__ __launch_bounds__(kBlock) void k_cell_box(const Pt<XY>* __restrict__ pts,
                                                    const int32_t* __restrict__ cell_start,
                                                    const int32_t* __restrict__ occ,
                                                    const int32_t* __restrict__ n_occ, Geom g,
                                                    uint8_t* __restrict__ mutual,
                                                    CellRec<D>* __restrict__ crec,
                                                    unsigned long long* __restrict__ cmin =
                                                        nullptr,
                                                    const int32_t* __restrict__ sorig = nullptr,
                                                    const float2* __restrict__ slab_t = nullptr) {
  static_assert(!XY || D == 2, "xy points are 2-D");
  // sorig (kernel-uniform): cmin[c] = the (min original, sorted) pair over ALL the cell's points
  // (the fused K5 keeps it for all-core cells), read alongside the points; otherwise none (~0)
  constexpr int L = kCbLanes;
  const int j = threadIdx.x & (L - 1);
  const int64_t no = *n_occ;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t - j < no * L;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = t / L;
    const bool act = q < no;
    int c = 0, b = 0, e = 0;
    if (act) {
      c = occ[q];
      b = cell_start[c];
      e = cell_start[c + 1];
    }
    float x0 = FLT_MAX, x1 = -FLT_MAX, y0 = FLT_MAX, y1 = -FLT_MAX;
    float z0 = FLT_MAX, z1 = -FLT_MAX, t0 = FLT_MAX, t1 = -FLT_MAX;
    uint64_t mn = ~0ull;
    // 8 loads in flight per lane: a dense cell (hundreds of points) is otherwise a chain of
    // dependent load round trips on its lanes
    constexpr int kU = 8;
    for (int s0 = b + j; s0 < e; s0 += L * kU) {
      float4 pp[kU];
      uint32_t so[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int s2 = s0 + L * u;
        const int sc = (s2 < e) ? s2 : s0;  // duplicates of a cell point leave the box as is
        pp[u] = load_pt<XY>(pts, sc);
        if (sorig) so[u] = (uint32_t)sorig[sc];
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float4 p = pp[u];
        x0 = fminf(x0, p.x); x1 = fmaxf(x1, p.x);
        y0 = fminf(y0, p.y); y1 = fmaxf(y1, p.y);
        if constexpr (!XY) {
          z0 = fminf(z0, p.z); z1 = fmaxf(z1, p.z);
          t0 = fminf(t0, p.w); t1 = fmaxf(t1, p.w);
        }
        if (sorig) {
          const int s2 = s0 + L * u;
          const uint64_t v = ((uint64_t)so[u] << 32) | (uint32_t)((s2 < e) ? s2 : s0);
          mn = v < mn ? v : mn;
        }
      }
    }
    // (the cell loop is uniform over the aligned 16-lane group: all its lanes are active)
    if (sorig) mn = row_reduce<L>(mn, OpMin{});
    x0 = row_reduce<L>(x0, OpMin{}); x1 = row_reduce<L>(x1, OpMax{});
    y0 = row_reduce<L>(y0, OpMin{}); y1 = row_reduce<L>(y1, OpMax{});
    if constexpr (XY) {
      t0 = t1 = slab_t[g.slab_of_key(c)].x;
    } else {
      z0 = row_reduce<L>(z0, OpMin{}); z1 = row_reduce<L>(z1, OpMax{});
      t0 = row_reduce<L>(t0, OpMin{}); t1 = row_reduce<L>(t1, OpMax{});
    }
    if (D != 3) {
      z0 = t0;  // 2-D: pts[].z carries t (unused by the 2-D tests)
      z1 = t1;
    }
    if (act && j == 0) {
      CellRec<D> r{};
      r.b = b;
      r.e = e;
      r.x0 = x0;
      r.x1 = x1;
      r.y0 = y0;
      r.y1 = y1;
      if constexpr (D == 3) {
        r.z0 = z0;
        r.z1 = z1;
      }
      r.t0 = t0;
      r.t1 = t1;
      crec[c] = r;
      const double dx = (double)x1 - (double)x0;
      const double dy = (double)y1 - (double)y0;
      double d2 = dx * dx + dy * dy;
      if (D == 3) {
        const double dz = (double)z1 - (double)z0;
        d2 = d2 + dz * dz;
      }
      const float dt = t1 - t0;
      mutual[c] = (d2 <= g.eps2 && dt <= g.epst) ? 1 : 0;
      if (cmin) cmin[c] = sorig ? mn : ~0ull;  // the core pass's per-cell minima
    }
  }
}

// The same records with the small cells one LANE each: a wave takes 64 consecutive occupied
// cells, every lane the box of its own cell when it holds at most kCbSmall points (its points
// loaded together, branch-free), then the wave's other cells four at a time at kCbLanes lanes
// each.  Clutter singletons (most of the occupied cells at the standard density) no longer take
// a 16-lane group each.
constexpr int kCbSmall = 4;
template <int D>
__device__ __forceinline__ void cell_box_store(int c, int b, int e, float x0, float x1, float y0,
                                               float y1, float z0, float z1, float t0, float t1,
                                               uint64_t mn, bool has_mn, const Geom& g,
                                               uint8_t* __restrict__ mutual,
                                               CellRec<D>* __restrict__ crec,
                                               unsigned long long* __restrict__ cmin) {
  CellRec<D> r{};
  r.b = b;
  r.e = e;
  r.x0 = x0;
  r.x1 = x1;
  r.y0 = y0;
  r.y1 = y1;
  if constexpr (D == 3) {
    r.z0 = z0;
    r.z1 = z1;
  }
  r.t0 = t0;
  r.t1 = t1;
  crec[c] = r;
  const double dx = (double)x1 - (double)x0;
  const double dy = (double)y1 - (double)y0;
  double d2 = dx * dx + dy * dy;
  if (D == 3) {
    const double dz = (double)z1 - (double)z0;
    d2 = d2 + dz * dz;
  }
  const float dt = t1 - t0;
  mutual[c] = (d2 <= g.eps2 && dt <= g.epst) ? 1 : 0;
  if (cmin) cmin[c] = has_mn ? mn : ~0ull;  // the core pass's per-cell minima
}

template <int D, bool XY = false>
__global__ __launch_bounds__(kBlock) void k_cell_box_mixed(const Pt<XY>* __restrict__ pts,
                                                          const int32_t* __restrict__ cell_start,
                                                          const int32_t* __restrict__ occ,
                                                          const int32_t* __restrict__ n_occ,
                                                          Geom g, uint8_t* __restrict__ mutual,
                                                          CellRec<D>* __restrict__ crec,
                                                          unsigned long long* __restrict__ cmin =
                                                              nullptr,
                                                          const int32_t* __restrict__ sorig =
                                                              nullptr,
                                                          const float2* __restrict__ slab_t =
                                                              nullptr) {
  static_assert(!XY || D == 2, "xy points are 2-D");
  constexpr int L = kCbLanes;
  const int lane = threadIdx.x & 63;
  const int grp = lane / L, j = lane & (L - 1);
  const int64_t no = *n_occ;
  if (no == 0) return;
  const int64_t wpb = kBlock / 64;
  for (int64_t q0 = ((int64_t)blockIdx.x * wpb + threadIdx.x / 64) * 64; q0 < no;
       q0 += (int64_t)gridDim.x * wpb * 64) {
    const int64_t q = q0 + lane;
    const bool act = q < no;
    const int c = occ[act ? q : no - 1];
    const int b = cell_start[c], e = cell_start[c + 1];
    const bool small = act && e - b <= kCbSmall;
    {  // this lane's cell when small (every lane loads: branch-free)
      float4 pp[kCbSmall];
      uint32_t so[kCbSmall];
#pragma unroll
      for (int u = 0; u < kCbSmall; ++u) {
        const int sc = (b + u < e) ? b + u : b;  // duplicates of a cell point leave the box as is
        pp[u] = load_pt<XY>(pts, sc);
        if (sorig) so[u] = (uint32_t)sorig[sc];
      }
      float x0 = FLT_MAX, x1 = -FLT_MAX, y0 = FLT_MAX, y1 = -FLT_MAX;
      float z0 = FLT_MAX, z1 = -FLT_MAX, t0 = FLT_MAX, t1 = -FLT_MAX;
      if constexpr (XY) t0 = t1 = slab_t[g.slab_of_key(c)].x;
      uint64_t mn = ~0ull;
#pragma unroll
      for (int u = 0; u < kCbSmall; ++u) {
        const float4 p = pp[u];
        x0 = fminf(x0, p.x); x1 = fmaxf(x1, p.x);
        y0 = fminf(y0, p.y); y1 = fmaxf(y1, p.y);
        if constexpr (!XY) {
          z0 = fminf(z0, p.z); z1 = fmaxf(z1, p.z);
          t0 = fminf(t0, p.w); t1 = fmaxf(t1, p.w);
        }
        if (sorig) {
          const uint64_t v = ((uint64_t)so[u] << 32) | (uint32_t)((b + u < e) ? b + u : b);
          mn = v < mn ? v : mn;
        }
      }
      if (D != 3) {
        z0 = t0;  // 2-D: pts[].z carries t
        z1 = t1;
      }
      if (small)
        cell_box_store<D>(c, b, e, x0, x1, y0, y1, z0, z1, t0, t1, mn, sorig != nullptr, g,
                          mutual, crec, cmin);
    }
    // the wave's other cells, four at a time (group grp takes the grp-th of them)
    uint64_t big = __ballot(act && !small);
    while (big) {  // (wave-uniform)
      int pick = -1;
#pragma unroll
      for (int k = 0; k < 64 / L; ++k) {
        const int lk = big ? __ffsll((unsigned long long)big) - 1 : -1;
        if (grp == k) pick = lk;
        if (big) big &= big - 1;
      }
      // (every lane takes part in the shuffles: a conditional one would read inactive lanes)
      const int src = pick < 0 ? 0 : pick;
      const int cc = __shfl(c, src), bb = __shfl(b, src), es = __shfl(e, src);
      const int ee = pick < 0 ? bb : es;
      float x0 = FLT_MAX, x1 = -FLT_MAX, y0 = FLT_MAX, y1 = -FLT_MAX;
      float z0 = FLT_MAX, z1 = -FLT_MAX, t0 = FLT_MAX, t1 = -FLT_MAX;
      uint64_t mn = ~0ull;
      constexpr int kU = 8;  // loads in flight per lane (as k_cell_box)
      for (int s0 = bb + j; s0 < ee; s0 += L * kU) {
        float4 pp[kU];
        uint32_t so[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int s2 = s0 + L * u;
          const int sc = (s2 < ee) ? s2 : s0;
          pp[u] = load_pt<XY>(pts, sc);
          if (sorig) so[u] = (uint32_t)sorig[sc];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float4 p = pp[u];
          x0 = fminf(x0, p.x); x1 = fmaxf(x1, p.x);
          y0 = fminf(y0, p.y); y1 = fmaxf(y1, p.y);
          if constexpr (!XY) {
            z0 = fminf(z0, p.z); z1 = fmaxf(z1, p.z);
            t0 = fminf(t0, p.w); t1 = fmaxf(t1, p.w);
          }
          if (sorig) {
            const int s2 = s0 + L * u;
            const uint64_t v = ((uint64_t)so[u] << 32) | (uint32_t)((s2 < ee) ? s2 : s0);
            mn = v < mn ? v : mn;
          }
        }
      }
      if (sorig) mn = row_reduce<L>(mn, OpMin{});
      x0 = row_reduce<L>(x0, OpMin{}); x1 = row_reduce<L>(x1, OpMax{});
      y0 = row_reduce<L>(y0, OpMin{}); y1 = row_reduce<L>(y1, OpMax{});
      if constexpr (XY) {
        t0 = t1 = slab_t[g.slab_of_key(cc)].x;
      } else {
        z0 = row_reduce<L>(z0, OpMin{}); z1 = row_reduce<L>(z1, OpMax{});
        t0 = row_reduce<L>(t0, OpMin{}); t1 = row_reduce<L>(t1, OpMax{});
      }
      if (D != 3) {
        z0 = t0;
        z1 = t1;
      }
      if (pick >= 0 && j == 0)
        cell_box_store<D>(cc, bb, ee, x0, x1, y0, y1, z0, z1, t0, t1, mn, sorig != nullptr, g,
                          mutual, crec, cmin);
    }
  }
}

// Actual time range per slab from its occupied cells' records (slabs are the slowest key
// dimension: a slab's cells are a contiguous range of the ascending occupied-cell list, found
// through the head-flag scan at the slab's first point).  One block per slab.
template <int D>
__global__ __launch_bounds__(kBlock) void k_slab_range(const CellRec<D>* __restrict__ crec,
                                                      const int32_t* __restrict__ occ,
                                                      const int32_t* __restrict__ hpos,
                                                      const int32_t* __restrict__ cell_start,
                                                      int64_t cells_per_slab, int nt,
                                                      float2* __restrict__ slab_t,
                                                      const int32_t* __restrict__ occ_base) {
  const int s = blockIdx.x;
  if (s >= nt) return;
  const int q0 = occ_base ? occ_base[s] : hpos[cell_start[(int64_t)s * cells_per_slab]];
  const int q1 = occ_base ? occ_base[s + 1] : hpos[cell_start[(int64_t)(s + 1) * cells_per_slab]];
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (int q = q0 + threadIdx.x; q < q1; q += blockDim.x) {
    const CellRec<D> r = crec[occ[q]];
    lo = fminf(lo, r.t0);
    hi = fmaxf(hi, r.t1);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  __shared__ float slo[kBlock / 64], shi[kBlock / 64];
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x / 64] = lo;
    shi[threadIdx.x / 64] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      lo = fminf(lo, slo[w]);
      hi = fmaxf(hi, shi[w]);
    }
    // empty slab: lo > hi, never matches
    slab_t[s] = make_float2(lo, hi);
  }
}
