// The A/B switches: RPT_* environment variables that select a replaced kernel form for same-box
// measurements.  They exist only in the A/B build (-DRPT_AB, librpt_ab.so, tools/ab_*.sh): the
// shipped librpt.so reads no environment and always runs the default forms the parity suite
// covers.  This header is the only place that names a switch; every read site takes its value
// from ab().  Host-only, no HIP include (tools/ab_switches_dump.cpp compiles it alone).
#pragma once
#include <cstdlib>

namespace rpt {

// three values: 0 off, 1 the default rule, 2 forced on (the parity tests of the A/B build run a
// path on inputs its default rule would not take it for)
inline int ab_tri(int v) { return (v == 0 || v == 2) ? v : 1; }
template <class T>
inline T ab_range(T v, T lo, T hi, T otherwise) {
  return (v >= lo && v <= hi) ? v : otherwise;
}

// X(name, member, type, default, value when set): `e` is the variable's text (never null there);
// an unset variable leaves the default.
//   off iff 0: std::atoi(e) != 0      on iff 1: std::atoi(e) == 1
#define RPT_AB_SWITCHES(X)                                                                        \
  /* K1 (polar.hip, the driver of the polar_*.inc kernels; stack.cpp, shard.cpp) */               \
  /* =0: K1 reads the echo twice (no staged kept samples from the count pass) */                  \
  X("RPT_K1_STAGE", k1_stage, bool, true, std::atoi(e) != 0)                                      \
  /* =0: the wave-per-group write instead of the persistent k_expand_write */                     \
  X("RPT_K1_EXPAND", k1_expand, bool, true, std::atoi(e) != 0)                                    \
  /* land filter (land.hip) */                                                                    \
  /* =0: the int32 + float64 atomics kernel also for u8 points */                                 \
  X("RPT_LAND_U8", land_u8, bool, true, std::atoi(e) != 0)                                        \
  /* K4, the grid build (stdbscan.hip build_t) */                                                 \
  /* =0: no f32 screen of the squared distances (off only for a leading '0') */                   \
  X("RPT_F32_SCREEN", f32_screen, bool, true, e[0] != '0')                                        \
  /* the 2-D cell side as a fraction of eps, 0.5 - 0.7 */                                         \
  X("RPT_CELL_SIDE", cell_side, double, 0.7, ab_range(std::atof(e), 0.5, 0.7, 0.7))               \
  /* =0: keys + radix sort + gather instead of the per-slab counting sort */                      \
  X("RPT_K4_BUCKET", k4_bucket, bool, true, std::atoi(e) != 0)                                    \
  /* =k: k blocks per slab (1 = the single-block k_slab_bucket); 0: by the default rule */        \
  X("RPT_SLAB_CHUNKS", slab_chunks, int, 0, std::atoi(e))                                         \
  /* =1: the one-block-per-slab k_slab_chunk_scan also with many chunks per slab */               \
  X("RPT_CHUNK_SCAN", chunk_scan, bool, false, std::atoi(e) == 1)                                 \
  /* =0: the fused K5's all-core cell minima from k_cell_box, not from k_slab_bucket */           \
  X("RPT_BUCKET_ALLMIN", bucket_allmin, int, 1, ab_tri(std::atoi(e)))                             \
  /* =0: 16 lanes for every cell's box (k_cell_box); 2: k_cell_box_mixed always */                \
  X("RPT_CELL_BOX_MIXED", cell_box_mixed, int, 1, ab_tri(std::atoi(e)))                           \
  /* =0: core labels scattered from sorted order (k_label_core); 2: the inverse permutation */    \
  /* and original-order labels at every density */                                                \
  X("RPT_LABEL_ORIG", label_orig, int, 1, ab_tri(std::atoi(e)))                                   \
  /* =0: sorted points stay float4 (no 8-byte xy layout) */                                       \
  X("RPT_XY_POINTS", xy_points, bool, true, std::atoi(e) != 0)                                    \
  /* caps the wave-per-item kernels' grids (>= 8; fewer resident waves leave room for other */    \
  /* stacks' kernels on the same CUs) */                                                          \
  X("RPT_WAVE_GRID_CAP", wave_grid_cap, int, 4096, std::atoi(e) >= 8 ? std::atoi(e) : 4096)       \
  /* K5, the core flags */                                                                        \
  /* 0 the round-1 queue pipeline, 2 cells + point-flag fill (no queue), else cells write */      \
  /* the point flags; the latter two end in k_core_slow_cells */                                  \
  X("RPT_K5_MODE", k5_mode, int, 0, std::atoi(e))                                                 \
  /* =1: the LDS-tile pass (k_core_tiles; measured slower) */                                     \
  X("RPT_K5_TILES", k5_tiles, bool, false, std::atoi(e) == 1)                                     \
  /* =0: the separate level-3 fill pass */                                                        \
  X("RPT_K5_FUSED", k5_fused, bool, true, std::atoi(e) != 0)                                      \
  /* =0: the slow pass re-classifies every window (k_core_slow) */                                \
  X("RPT_K5_MASK", k5_mask, bool, true, std::atoi(e) != 0)                                        \
  /* K6, the union passes */                                                                      \
  /* bit 0: no path halving, bit 1: XCD-aware item ranges (see XcdRange) */                       \
  X("RPT_UF_FLAGS", uf_flags, int, 2, std::atoi(e) & 3)                                           \
  /* =0: the second union pass enumerates every window */                                         \
  X("RPT_UNION_LIST", union_list, bool, true, std::atoi(e) != 0)                                  \
  /* =0: one cell per wave in the box-certain union pass */                                       \
  X("RPT_UNION_PAIR", union_pair, bool, true, std::atoi(e) != 0)                                  \
  /* =0: k_union over every point (not the listed cells') */                                      \
  X("RPT_UNION_NM", union_nm, bool, true, std::atoi(e) != 0)                                      \
  /* occupied cells per wave iteration of k_union_cells_pair, 1 - 64; 0: by the point count */    \
  X("RPT_UNION_CPW", union_cpw, int, 0, ab_range(std::atoi(e), 1, 64, 0))                         \
  /* =0: no root snapshot before the listed union pass; 2: also on dense slabs */                 \
  X("RPT_UNION_SNAP", union_snap, int, 1, ab_tri(std::atoi(e)))                                   \
  /* =1: a compression pass closes the union stage */                                             \
  X("RPT_UF_COMPRESS", uf_compress, bool, false, std::atoi(e) == 1)                               \
  /* =0: the per-point union init / component / core-label kernels also on grids whose cells */   \
  /* are all mutual */                                                                            \
  X("RPT_CELL_COMP", cell_comp, bool, true, std::atoi(e) != 0)                                    \
  /* =0: k_ccmin walks every core point's parent chain */                                         \
  X("RPT_CELL_ROOTS", cell_roots, bool, true, std::atoi(e) != 0)                                  \
  /* K7, the border labels */                                                                     \
  /* =1: K7 by LDS tiles (k_label_tiles; measured slower than k_label) */                         \
  X("RPT_K7_TILES", k7_tiles, bool, false, std::atoi(e) == 1)                                     \
  /* lanes per non-core point in k_label: 64, anything else 32 (two points per wave) */           \
  X("RPT_K7_W", k7_w, int, 32, std::atoi(e) == 64 ? 64 : 32)                                      \
  /* K9, the summaries (summaries.hip) */                                                         \
  /* =1: the radix sort, not the per-frame counting sort (on only for a leading '1') */           \
  X("RPT_K9_RADIX", k9_radix, bool, false, e[0] == '1')                                           \
  /* set at all, even to empty: the "[rpt stats]" diagnostics on stderr (they synchronise) */     \
  X("RPT_STATS", stats, bool, false, e != nullptr)

struct AbSwitches {
#define RPT_AB_MEMBER(name, member, type, dflt, when_set) type member = dflt;
  RPT_AB_SWITCHES(RPT_AB_MEMBER)
#undef RPT_AB_MEMBER
};

#ifdef RPT_AB
// get(name): the variable's text or null (std::getenv, or a test's own table)
inline AbSwitches ab_parse(const char* (*get)(const char*)) {
  AbSwitches s;
#define RPT_AB_PARSE(name, member, type, dflt, when_set) \
  if (const char* e = get(name)) s.member = (when_set);
  RPT_AB_SWITCHES(RPT_AB_PARSE)
#undef RPT_AB_PARSE
  return s;
}
inline const AbSwitches& ab() {  // parsed once per process
  static const AbSwitches s =
      ab_parse([](const char* name) -> const char* { return std::getenv(name); });
  return s;
}
#else
inline constexpr AbSwitches kAbDefaults{};
inline const AbSwitches& ab() { return kAbDefaults; }  // constants the compiler folds
#endif

}  // namespace rpt
