// Shard driver, representatives and the packed result.  Reads shard_shared.inc (WinIds, lookup),
// shard_pack.h (kHdr, kPackMagic) and stack_impl.h (SegPack).
//   rpt_shard_finish  k_reps_keys -> k_root_reps -> [scan of the word counts] -> k_reps_write:
//                     read the merge table and ST-DBSCAN's union-find arrays, leave rep (per root)
//                     and reps (the sorted representative list; its length behind the scan);
//                     after the global label pass and K9, k_shard_pack: reads the segment arrays,
//                     reps and the K1 file offsets, leaves everything rank 0 needs in out
//   rpt_shard_labels  k_map_labels: the own points' local labels through rank 0's map

// Flags of the representative list, one bit per entry k < keys_cap + n: the merge table's class
// minima below the window (external representatives) here -- a wave per 64 entries writes their
// two words and popcounts, which also clears the window part of both -- and the window points
// that are their own representative by k_root_reps after it.  The list's order comes from a
// scan over the (keys_cap + n) / 32 word counts.
__global__ void k_reps_keys(int64_t n, WinIds w, const int64_t* __restrict__ keys,
                            const int64_t* __restrict__ vals, const int64_t* __restrict__ meta,
                            int64_t keys_cap, uint32_t* __restrict__ bits,
                            int32_t* __restrict__ wcnt) {
  const int64_t m = meta[0] > 0 ? meta[0] : 0;
  const int64_t wstart = w.gid(0);
  const int lane = threadIdx.x & 63;
  const int64_t total = keys_cap + n;
  for (int64_t c0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; c0 < total;
       c0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = c0 + lane;
    const bool f = k < keys_cap && k < m && keys[k] == vals[k] && keys[k] < wstart;
    const uint64_t b = __ballot(f);
    if (lane < 2) {
      const uint32_t word = (uint32_t)(b >> (32 * lane));
      bits[(c0 >> 5) + lane] = word;
      wcnt[(c0 >> 5) + lane] = __popc(word);
    }
  }
}

// Per ROOT of the window's core components (a core point s with parent[s] == s; its window
// index i = sorig[s] is the component's id, its minimum original index): rep[i] = the global
// representative (the merge table's class minimum of gid(i), else gid(i) itself) -- the only
// entries of rep the global label pass reads -- and, when the root is its own representative,
// its list flag (after k_reps_keys).  Components are few: the atomics are rare.  Replaces a
// representative per window point (which needed every point's component id).
__global__ void k_root_reps(const uint8_t* __restrict__ core, const int32_t* __restrict__ parent,
                            const int32_t* __restrict__ sorig, int64_t n, WinIds w,
                            const int64_t* __restrict__ keys, const int64_t* __restrict__ vals,
                            const int64_t* __restrict__ meta, int64_t keys_cap,
                            int64_t* __restrict__ rep, uint32_t* __restrict__ bits,
                            int32_t* __restrict__ wcnt) {
  const int64_t m = meta[0] > 0 ? meta[0] : 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const uint8_t c = core[s];  // (both loads issued together)
    const int32_t p = parent[s];
    if (!c || p != (int32_t)s) continue;
    const int32_t i = sorig[s];
    const int64_t g = w.gid(i);
    const int64_t r = lookup(keys, vals, m, g);
    rep[i] = r;
    if (r == g) {
      const int64_t k = keys_cap + i;
      atomicOr(&bits[k >> 5], 1u << (k & 31));
      atomicAdd(&wcnt[k >> 5], 1);
    }
  }
}

__global__ void k_reps_write(const uint32_t* __restrict__ bits, const int64_t* __restrict__ wpre,
                             int64_t keys_cap, int64_t n, WinIds w,
                             const int64_t* __restrict__ keys, int64_t* __restrict__ reps) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < keys_cap + n;
       k += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t word = bits[k >> 5];
    const uint32_t bit = 1u << (k & 31);
    if (word & bit)
      reps[wpre[k >> 5] + __popc(word & (bit - 1u))] = k < keys_cap ? keys[k] : w.gid(k - keys_cap);
  }
}

// Everything rank 0 needs from this rank, at fixed offsets of a buffer of cap int64 words:
//   [magic, S, n_reps, flags, words, F, frame0, kept] [built F] [first noise F]
//   [count S] [first S] [frame << 32 | label S] [cx | cy << 32 S] [mi S] [reps n_reps]
// flags: 1 this rank's pairs exceeded their capacity, 2 the merge ran on too many ids (host
// merge), 4 the buffer is too small (words holds the size needed).  S = -1: a frame held more
// labels than K9's frame sort takes (redo on the radix path).
__global__ void k_shard_pack(const int32_t* __restrict__ n_seg_dev, const int64_t* __restrict__ nr,
                             const int64_t* __restrict__ mmeta, const int64_t* __restrict__ pairs,
                             int64_t pair_cap, SegPack a, const int64_t* __restrict__ reps,
                             const int64_t* __restrict__ file_off, int32_t G, int32_t F,
                             int64_t frame0, int64_t kept, int64_t* __restrict__ out,
                             int64_t cap) {
  const int64_t S = n_seg_dev ? (int64_t)*n_seg_dev : 0;
  const int64_t R = *nr;
  const int64_t Sp = S > 0 ? S : 0;
  const int64_t words = kHdr + 2 * (int64_t)F + 5 * Sp + R;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (i0 == 0) {
    int64_t fl = 0;
    if (pairs && pairs[0] > pair_cap) fl |= 1;
    if (mmeta && (mmeta[1] != 0)) fl |= 1;
    if (mmeta && mmeta[0] < 0) fl |= 2;
    if (words > cap) fl |= 4;
    out[0] = kPackMagic;
    out[1] = S;
    out[2] = R;
    out[3] = fl;
    out[4] = words;
    out[5] = F;
    out[6] = frame0;
    out[7] = kept;
  }
  if (words > cap) return;
  int64_t* built = out + kHdr;
  int64_t* noise = built + F;
  int64_t* cnt = noise + F;
  int64_t* first = cnt + Sp;
  int64_t* fl = first + Sp;
  int64_t* cxy = fl + Sp;
  int64_t* mi = cxy + Sp;
  int64_t* rp = mi + Sp;
  for (int64_t f = i0; f < F; f += step) {
    built[f] = file_off[(int64_t)(f + 1) * G] > file_off[(int64_t)f * G] ? 1 : 0;
    noise[f] = a.noise[f];
  }
  for (int64_t s = i0; s < Sp; s += step) {
    cnt[s] = a.count[s];
    first[s] = a.first[s];
    fl[s] = ((int64_t)a.frame[s] << 32) | (int64_t)(uint32_t)a.label[s];
    cxy[s] = (int64_t)(((uint64_t)__float_as_uint(a.cy[s]) << 32) |
                       (uint64_t)__float_as_uint(a.cx[s]));
    mi[s] = (int64_t)(uint64_t)__float_as_uint(a.mi[s]);
  }
  for (int64_t r = i0; r < R; r += step) rp[r] = reps[r];
}

__global__ void k_map_labels(const int32_t* __restrict__ lab, int64_t n,
                             const int32_t* __restrict__ map, int64_t nr,
                             int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = lab[i];
    out[i] = (l >= 0 && l < nr) ? map[l] : -1;
  }
}
