// knobs.h -- what the library reads from the environment, in one place.
//
// SUPPORTED (documented in INTEGRATION.md section 5; read where they act, with std::getenv):
//   NGSLD_REPLAY, NGSLD_REPLAY_DEVICE, NGSLD_REPLAY_SKIP, NGSLD_REPLAY_THREADS, NGSLD_EXACT_STORE   the exact-order replay
//   NGSLD_PAIR_KERNEL                                                                              kernel family override
//   NGSLD_GZ_LEVEL, NGSLD_HOST_TEXT, NGSLD_PIPELINE, NGSLD_PIN_REGISTER                             the drop-in binary / writer
//   NGSLD_TRACE, NGSLD_TIMING, NGSLD_ROCTX, NGSLD_MULTI_VERBOSE                                     diagnostics
//
// TEST-ONLY fault injectors and shapes (tests/ set them; nothing else should): NGSLD_TEST_<NAME>, read through test_knob("<NAME>").
// They force the paths a healthy box never takes -- a host that cannot pin, a device without room, launches cut into many
// grids, batches of a few hundred rows -- so that the suite can hold those paths to the same records.
//   BATCH_PAIRS, STAGE_BYTES, MAX_BLOCKS, PIN_LIMIT_BYTES, PREP_EXACT, HARD_KERNEL, SLAB_SITES, MULTI_DIST,
//   RUN_DIRECT, RUN_TAPER, RUN_STREAMS, TAIL_LEN, TAIL_PAIRS, TILES, TILE_MIN_MB,
//   TEXT_STREAMS, TEXT_HOST_PATCH, TEXT_HOST_PATCH_FAIL_EVERY, TEXT_FALLBACK_EVERY,
//   TEXT_GROUPS, TEXT_GROUP_PAIRS,
//   EXACT_CHUNK_SITES, EXACT_SLOW_US, EXACT_STORE_NO_ROOM, REPLAY_LIST_CAP, REPLAY_SOURCE, LANE_ITER_CAP,
//   PRUNE_HOST_AFTER, DECAY_LDS_BYTES, DECAY_CHUNK_PAIRS, BLOCKS_CHUNK_PAIRS, BLOCKS_HOST_ROWS, BLOCKS_TEXT_ROWS,
//   SITE_LDS_BYTES, SITE_CHUNK_PAIRS, CLUSTER_CHUNK_PAIRS, GRID_LDS_BYTES, GRID_CHUNK_PAIRS,
//   LINKED_CHUNK_PAIRS, LINKED_FORCE_HOST, SCAN_CHUNK_PAIRS, SCAN_PLANT_DP,
//   PRUNE_CHUNK_PAIRS, RECORD_SLICE_ITEMS, SUM_WRAP_LIMIT, ANALYZE_CHUNK_PAIRS,
//   FIRST_STEP, PAIR_MOMENTS, MOMENTS_PAIRS, PARTNERS_CHUNK_PAIRS, PARTNERS_PLANT_DP,
//   DMAP_CHUNK_PAIRS, DMAP_LDS_BYTES,
//   CROSS_CHUNK_PAIRS, CROSS_SPAN_ITEMS, CROSS_PLANT_DP,
//   TREE_CHUNK_PAIRS, TREE_PLANT
// TREE_CHUNK_PAIRS=n: ngsld_ld_tree's chunks of rows hold about n pairs instead of 2^24 (tree.hip).  TREE_PLANT=R:X: SCAN_PLANT_DP for
// ngsld_ld_tree, into the field the call reads.
// CROSS_CHUNK_PAIRS=n: ngsld_cross_ld's chunks of rows hold about n pairs instead of 2^24 (cross.hip).  CROSS_SPAN_ITEMS=M: a
// wavefront of its kernel carries its current cell over M consecutive items instead of the measured default (CROSS.md); 1 is one
// set of atomics per run, grid.hip's global form.  CROSS_PLANT_DP=R:X: SCAN_PLANT_DP for ngsld_cross_ld.
// DMAP_CHUNK_PAIRS=n: ngsld_decay_map's chunks of rows hold about n pairs instead of 2^24 (decay_map.hip).  DMAP_LDS_BYTES=n: its
// per-workgroup LDS budget for the home group's bins, at most 64 KiB; 0 sends every add to global memory.
// PARTNERS_PLANT_DP=R:X: SCAN_PLANT_DP for ngsld_partners (partners.hip), whose refusal begins at 2^31 micro-units.
// LINKED_FORCE_HOST=1: every chunk of ngsld_linked_pairs takes the host formatter, as BLOCKS_HOST_ROWS does for the block matrices.
// SCAN_PLANT_DP=R:X: record R of the plan gets D' = X in ngsld_scan's record buffer before its kernel reads it (scan.hip) -- no input
// gives a finite D' near 2^38 micro-units, and the refusal of one has to be reached somehow.
// PRUNE_CHUNK_PAIRS, RECORD_SLICE_ITEMS and SUM_WRAP_LIMIT bring the large-job paths of the record passes (record_pass.h) down to jobs of a few thousand pairs, where
// tests/test_gpu_record_pass_large.py holds them to the passes' rules: ngsld_prune's chunk loop (its edge arrays regrown and its
// edge count carried from chunk to chunk; a row that does not fit the record buffer), a chunk's items cut into several launches
// (2^24 items otherwise), and the guard of the integer sums (max |q| tracked from 2^25 rows on, refused from 2^63 on).
// ANALYZE_CHUNK_PAIRS: the chunk of ngsld_analyze (analyze.hip), which does not read the single calls' *_CHUNK_PAIRS.
// FIRST_STEP=0: the run kernel takes no pair's first EM step from the sites' dosages (ld_kernel_run.h) -- every pair starts at
// iteration 0 with the per-individual step, and the records are what they were before that step existed (A/B, tests).
// PAIR_MOMENTS=0: no pair_ld_moments_kernel in front of the run kernel (engine_run.hip, timed_launch) -- the kernel forms each pair's
// Pearson cross moment and first-step dosage sum itself, and the records are what they were before the pass existed (A/B, tests;
// one exception, a site whose lane product of dens underflows: site_dose_kernel, ld_prep.hip).
// MOMENTS_PAIRS=n: the pass's array holds at most n pairs (never less than a row's), so a launch's rows are cut into several grids.
// (The knobs of closed A/B experiments -- lane caps and waves, sort-key tilings, run lengths, tile rows, text batch sizes -- are
// gone; their measurements are in HISTORY.md.)
#pragma once

#include <cstdlib>
#include <cstring>
#include <string>

namespace ngsld {

inline const char *test_knob(const char *name) {
  std::string key = "NGSLD_TEST_";
  key += name;
  return std::getenv(key.c_str());
}
inline bool test_knob_is(const char *name, const char *value) {
  const char *v = test_knob(name);
  return v != nullptr && std::strcmp(v, value) == 0;
}

}  // namespace ngsld
