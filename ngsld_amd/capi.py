"""ctypes binding of the C-ABI in include/ngsld.h and include/ngsld_host.h (libngsld.so, built in-tree).

This is plumbing: every call goes straight into the HIP library.  There is no Python or CPU fallback --
if the library is missing or no gfx950 device is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("NGSLD_LIB") or os.path.join(PKG_DIR, "libngsld.so")  # NGSLD_LIB: A/B builds of the same C-ABI
CLI_PATH = os.path.join(PKG_DIR, "bin", "ngsLD")

OK, ERR_INVALID, ERR_DEVICE, ERR_NOMEM, ERR_NAN, ERR_MAF_RANGE, ERR_SINK, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7


class Params(C.Structure):
    _fields_ = [("max_kb_dist", C.c_uint64), ("max_snp_dist", C.c_uint64), ("min_maf", C.c_double),
                ("ignore_miss_data", C.c_int32), ("extend_out", C.c_int32), ("rnd_sample", C.c_double),
                ("seed", C.c_uint64), ("first_row", C.c_uint64)]


class GenoOpts(C.Structure):
    _fields_ = [("log_scale", C.c_int32), ("ignore_miss_data", C.c_int32), ("on_device", C.c_int32),
                ("text_semantics", C.c_int32), ("call_geno", C.c_int32), ("per_individual_only", C.c_int32),
                ("N_thresh", C.c_double), ("call_thresh", C.c_double)]


REC_STD = np.dtype([("r2_ExpG", "<f8"), ("D", "<f8"), ("Dp", "<f8"), ("r2", "<f8")])
REC_EXT = np.dtype([("hap", "<f8", (4,)), ("n_ind_data", "<u4"), ("n_iter", "<u4")])


ITEM = np.dtype([("s1", "<u4"), ("s2_begin", "<u4"), ("count", "<u4"), ("reserved", "<u4"), ("mask", "<u8"),
                 ("first_record", "<u8")])


class Batch(C.Structure):
    _fields_ = [("s1_begin", C.c_uint64), ("s1_end", C.c_uint64), ("n_pairs", C.c_uint64), ("n_items", C.c_uint64),
                ("items", C.c_void_p), ("std", C.c_void_p), ("ext", C.c_void_p), ("text", C.c_void_p),
                ("text_len", C.c_uint64)]


def items_to_pairs(items: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(s1, s2) of every record described by an item array, in record order."""
    if len(items) == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    bits = (items["mask"][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    bits &= (np.arange(64)[None, :] < items["count"][:, None]).astype(np.uint64)
    idx, c = np.nonzero(bits)
    return items["s1"][idx].astype(np.uint64), (items["s2_begin"][idx].astype(np.uint64) + c.astype(np.uint64))


def items_from_pairs(s1: np.ndarray, s2: np.ndarray, span: int = 64) -> np.ndarray:
    """Build an item array for a list of pairs sorted by (s1, s2): chunks of `span` candidates from s1 + 1."""
    s1, s2 = np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)
    chunk = (s2 - s1 - 1) // span
    key = s1 * (1 << 32) + chunk
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    items = np.zeros(len(uniq), dtype=ITEM)
    items["s1"] = s1[first]
    items["s2_begin"] = s1[first] + 1 + chunk[first] * span
    items["first_record"] = first
    np.bitwise_or.at(items["mask"], inv, np.uint64(1) << (s2 - items["s2_begin"][inv]).astype(np.uint64))
    last = np.zeros(len(uniq), dtype=np.int64)
    np.maximum.at(last, inv, s2 - items["s2_begin"][inv].astype(np.int64))
    items["count"] = last + 1
    return items


SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Batch))
MULTI_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(Batch))
READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)
SLAB = np.dtype([("row_begin", "<u8"), ("row_end", "<u8"), ("site_end", "<u8")])

# every symbol the two headers declare (checked by tests/test_abi.py against the headers' text)
SYMBOLS = [
    "ngsld_version", "ngsld_create", "ngsld_destroy", "ngsld_last_error", "ngsld_set_geno_raw",
    "ngsld_set_geno_raw_opts", "ngsld_set_geno_lkl",
    "ngsld_get_maf", "ngsld_set_pos_dist", "ngsld_plan", "ngsld_plan_rows", "ngsld_run", "ngsld_run_device", "ngsld_set_text_output",
    "ngsld_set_replay_source", "ngsld_set_replay_matrix", "ngsld_set_replay", "ngsld_replay_stats", "ngsld_finish_device",
    "ngsld_set_exact_store", "ngsld_replay_info",
    "ngsld_plan_parts", "ngsld_run_multi", "ngsld_multi_last_distribution", "ngsld_rccl_selftest",
    "ngsld_last_kernel_time", "ngsld_pair_kernel", "ngsld_describe_dispatch", "ngsld_set_tuning", "ngsld_selftest", "ngsld_selftest_format",
    "ngsld_selftest_printed", "ngsld_reserve_text_buffers",
    "ngsld_window_ends", "ngsld_plan_slabs", "ngsld_slab_sites_for_budget", "ngsld_sites_for_budget", "ngsld_streamed_replay_info", "ngsld_set_memory_budget", "ngsld_device_memory", "ngsld_run_streamed", "ngsld_run_streamed_text",
    "ngsld_host_read_geno_bin_range",
    "ngsld_host_set_threads", "ngsld_host_read_pos", "ngsld_host_pos_dist", "ngsld_host_label", "ngsld_host_free_pos", "ngsld_host_pos_slice",
    "ngsld_host_geno_size_ok", "ngsld_host_read_geno_bin", "ngsld_host_read_geno_text", "ngsld_host_format_header", "ngsld_host_format_pair",
    "ngsld_host_format_double", "ngsld_host_write_batch", "ngsld_host_replay_pair", "ngsld_host_missing_call_log",
    "ngsld_host_gz_open", "ngsld_host_gz_close",
    "ngsld_prune", "ngsld_host_prune_graph", "ngsld_host_prune_label",
    "ngsld_decay", "ngsld_decay_bins", "ngsld_host_decay_fit",
    "ngsld_blocks", "ngsld_blocks_sites", "ngsld_blocks_matrix", "ngsld_blocks_text",
    "ngsld_site_ld", "ngsld_site_ld_get",
    "ngsld_clusters", "ngsld_clusters_sites", "ngsld_clusters_table",
    "ngsld_grid", "ngsld_grid_cells", "ngsld_grid_chromosomes", "ngsld_grid_get",
    "ngsld_linked_pairs",
    "ngsld_scan", "ngsld_scan_get",
    "ngsld_analyze",
    "ngsld_partners", "ngsld_partners_info", "ngsld_partners_get",
    "ngsld_decay_map", "ngsld_decay_map_chromosomes", "ngsld_decay_map_groups", "ngsld_decay_map_bins",
    "ngsld_cross_ld", "ngsld_cross_ld_cells", "ngsld_cross_ld_chromosomes", "ngsld_cross_ld_get",
    "ngsld_ld_tree", "ngsld_ld_tree_merges", "ngsld_ld_tree_cut",
]


class ReplayStats(C.Structure):
    """ngsld_replay_stats_t (include/ngsld.h)."""
    _fields_ = [("pairs_flagged", C.c_uint64), ("pairs_replayed", C.c_uint64), ("pairs_on_device", C.c_uint64),
                ("pairs_on_host", C.c_uint64), ("sites_reevaluated", C.c_uint64), ("exact_store", C.c_int32),
                ("text_rows_patched", C.c_int32), ("exact_store_build_s", C.c_double), ("sites_degenerate", C.c_uint64)]


class PruneParams(C.Structure):
    """ngsld_prune_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("field", C.c_int32), ("max_kb_dist", C.c_double), ("min_weight", C.c_double),
                ("weight_type", C.c_int32), ("keep_heavy", C.c_int32), ("precision", C.c_int32), ("reserved", C.c_int32),
                ("subset", C.POINTER(C.c_char_p)), ("n_subset", C.c_uint64)]


class PruneStats(C.Structure):
    """ngsld_prune_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("nodes", C.c_uint64),
                ("edges", C.c_uint64), ("kept", C.c_uint64), ("excluded", C.c_uint64), ("rounds", C.c_uint64),
                ("host_nodes", C.c_uint64), ("host_edges", C.c_uint64), ("host_steps", C.c_uint64),
                ("pairs_ms", C.c_double), ("edges_ms", C.c_double), ("graph_ms", C.c_double), ("rounds_ms", C.c_double),
                ("host_ms", C.c_double), ("total_ms", C.c_double)]


class DecayParams(C.Structure):
    """ngsld_decay_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("bin_size", C.c_double), ("max_kb_dist", C.c_double),
                ("min_maf", C.c_double)]


class DecayStats(C.Structure):
    """ngsld_decay_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("lds", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("bins", C.c_uint64), ("bin_slots", C.c_uint64), ("chunks", C.c_uint64), ("pairs_ms", C.c_double),
                ("bin_ms", C.c_double), ("total_ms", C.c_double)]


class DecayMapParams(C.Structure):
    """ngsld_decay_map_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("bin_size", C.c_double), ("max_kb_dist", C.c_double),
                ("min_maf", C.c_double), ("window", C.c_uint64)]


class DecayMapStats(C.Structure):
    """ngsld_decay_map_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("lds", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("groups", C.c_uint64), ("bins", C.c_uint64), ("group_slots", C.c_uint64), ("bin_slots", C.c_uint64),
                ("chunks", C.c_uint64), ("pairs_ms", C.c_double), ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


class CrossLdParams(C.Structure):
    """ngsld_cross_ld_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("bin_size", C.c_uint64), ("min_maf", C.c_double),
                ("linked_min", C.c_double), ("min_kb_dist", C.c_double), ("abs_value", C.c_int32), ("within", C.c_int32)]


class CrossLdStats(C.Structure):
    """ngsld_cross_ld_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("lds", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("pairs_cross", C.c_uint64), ("cells", C.c_uint64), ("bins", C.c_uint64), ("chunks", C.c_uint64),
                ("span_items", C.c_uint64), ("pairs_ms", C.c_double), ("cross_ms", C.c_double), ("total_ms", C.c_double)]


class BlocksParams(C.Structure):
    """ngsld_blocks_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("chr", C.c_char_p), ("start", C.c_uint64),
                ("end", C.c_uint64)]


class BlocksStats(C.Structure):
    """ngsld_blocks_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("members", C.c_uint64), ("sites", C.c_uint64),
                ("pairs", C.c_uint64), ("pairs_in_region", C.c_uint64), ("cells_na", C.c_uint64), ("host_rows", C.c_uint64),
                ("chunks", C.c_uint64), ("pairs_ms", C.c_double), ("scatter_ms", C.c_double), ("format_ms", C.c_double),
                ("total_ms", C.c_double)]


class SiteLdParams(C.Structure):
    """ngsld_site_ld_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("max_kb_dist", C.c_double), ("min_maf", C.c_double),
                ("linked_min", C.c_double), ("abs_value", C.c_int32), ("reserved", C.c_int32)]


class SiteLdStats(C.Structure):
    """ngsld_site_ld_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("lds", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("sites_with_pairs", C.c_uint64), ("chunks", C.c_uint64), ("pairs_ms", C.c_double), ("site_ms", C.c_double),
                ("total_ms", C.c_double)]


class ClustersParams(C.Structure):
    """ngsld_clusters_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("field", C.c_int32), ("max_kb_dist", C.c_double), ("min_maf", C.c_double),
                ("min_weight", C.c_double), ("abs_value", C.c_int32), ("reserved", C.c_int32)]


class ClustersStats(C.Structure):
    """ngsld_clusters_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("nodes", C.c_uint64),
                ("edges", C.c_uint64), ("clusters", C.c_uint64), ("clusters_multi", C.c_uint64), ("largest", C.c_uint64),
                ("chunks", C.c_uint64), ("union_launches", C.c_uint64), ("pairs_ms", C.c_double), ("union_ms", C.c_double),
                ("finish_ms", C.c_double), ("total_ms", C.c_double)]


class TreeParams(C.Structure):
    """ngsld_ld_tree_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("field", C.c_int32), ("max_kb_dist", C.c_double), ("min_maf", C.c_double),
                ("min_weight", C.c_double), ("abs_value", C.c_int32), ("reserved", C.c_int32)]


class TreeStats(C.Structure):
    """ngsld_ld_tree_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("nodes", C.c_uint64),
                ("edges", C.c_uint64), ("merges", C.c_uint64), ("clusters", C.c_uint64), ("chunks", C.c_uint64),
                ("rounds", C.c_uint64), ("max_rounds", C.c_uint64), ("displaced", C.c_uint64), ("pairs_ms", C.c_double),
                ("edges_ms", C.c_double), ("reduce_ms", C.c_double), ("finish_ms", C.c_double), ("total_ms", C.c_double)]


class GridParams(C.Structure):
    """ngsld_grid_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("bin_size", C.c_uint64), ("max_kb_dist", C.c_double),
                ("min_maf", C.c_double), ("linked_min", C.c_double), ("abs_value", C.c_int32), ("reserved", C.c_int32)]


class GridStats(C.Structure):
    """ngsld_grid_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("lds", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("cells", C.c_uint64), ("bins", C.c_uint64), ("band", C.c_uint64), ("chunks", C.c_uint64),
                ("pairs_ms", C.c_double), ("grid_ms", C.c_double), ("total_ms", C.c_double)]


class LinkedParams(C.Structure):
    """ngsld_linked_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("field", C.c_int32), ("min_weight", C.c_double), ("max_kb_dist", C.c_double),
                ("min_maf", C.c_double), ("abs_value", C.c_int32), ("want", C.c_int32)]


class PartnersParams(C.Structure):
    """ngsld_partners_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("field", C.c_int32), ("abs_value", C.c_int32),
                ("min_weight", C.c_double), ("max_kb_dist", C.c_double), ("min_maf", C.c_double)]


class PartnersStats(C.Structure):
    """ngsld_partners_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("rows_counted", C.c_uint64),
                ("sites_with_partners", C.c_uint64), ("entries", C.c_uint64), ("chunks", C.c_uint64), ("pairs_ms", C.c_double),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


class ScanParams(C.Structure):
    """ngsld_scan_params (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("fields", C.c_uint32), ("half_window", C.c_uint64), ("max_kb_dist", C.c_double),
                ("min_maf", C.c_double), ("reserved", C.c_uint64)]


class ScanStats(C.Structure):
    """ngsld_scan_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("pairs_counted", C.c_uint64),
                ("largest_window", C.c_uint64), ("chunks", C.c_uint64), ("pairs_ms", C.c_double), ("scan_ms", C.c_double),
                ("total_ms", C.c_double)]


class Analysis(C.Structure):
    """ngsld_analysis (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("params", C.c_void_p), ("stats", C.c_void_p),
                ("labels", C.POINTER(C.c_char_p)), ("site_state", C.c_void_p)]


class AnalyzeStats(C.Structure):
    """ngsld_analyze_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_analyses", C.c_uint32), ("pairs", C.c_uint64), ("pairs_run", C.c_uint64),
                ("chunks", C.c_uint64), ("pairs_ms", C.c_double), ("kernels_ms", C.c_double), ("total_ms", C.c_double)]


# ngsld_analysis.kind, in the order of Engine.analyze's arguments
AN_PRUNE, AN_DECAY, AN_SITE_LD, AN_CLUSTERS, AN_GRID, AN_SCAN = 1, 2, 3, 4, 5, 6
ANALYSES = {"prune": AN_PRUNE, "decay": AN_DECAY, "site_ld": AN_SITE_LD, "clusters": AN_CLUSTERS, "grid": AN_GRID,
            "scan": AN_SCAN}


class _Job:
    """One analysis between its arguments and its result: the structs of its call (kept alive here), the single call, and
    read(), which fetches the result through the getters.  Engine.prune ... Engine.scan run call() then read(); Engine.analyze
    lists several jobs in one ngsld_analyze and reads each."""

    def __init__(self, kind, params, stats, call, read, labels=None, site_state=None):
        self.kind, self.params, self.stats, self.call, self.read = kind, params, stats, call, read
        self.labels, self.site_state = labels, site_state

    def run(self):
        self.call()
        return self.read()


class LinkedBatch(C.Structure):
    """ngsld_linked_batch (include/ngsld.h)."""
    _fields_ = [("n", C.c_uint64), ("s1", C.c_void_p), ("s2", C.c_void_p), ("std", C.c_void_p), ("ext", C.c_void_p),
                ("text", C.c_void_p), ("text_len", C.c_uint64)]


class LinkedStats(C.Structure):
    """ngsld_linked_stats (include/ngsld.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pairs", C.c_uint64), ("rows", C.c_uint64),
                ("text_bytes", C.c_uint64), ("host_rows", C.c_uint64), ("chunks", C.c_uint64), ("pairs_ms", C.c_double),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double), ("count_ms", C.c_double), ("scan_ms", C.c_double),
                ("write_ms", C.c_double)]


LINKED_RECORDS, LINKED_TEXT = 1, 2
LINKED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(LinkedBatch))
TEXT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)


class DecayFitResult(C.Structure):
    """ngsld_decay_fit_result (include/ngsld_host.h)."""
    _fields_ = [("rate", C.c_double), ("ld_max", C.c_double), ("ld_min", C.c_double), ("sse", C.c_double),
                ("n_bins", C.c_uint64)]


# the statistics LD decay bins, in TSV column order (bit k of ngsld_decay_params.fields = column 4 + k)
DECAY_FIELDS = ("r2_ExpG", "D", "Dp", "r2")


class NgsldError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ngsld error {code}: {msg}")
        self.code = code
        self.msg = msg


def build(force: bool = False, jobs: int = 8) -> None:
    """Compile the HIP library and the CLI in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(PKG_DIR, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", csrc, "clean"])
    subprocess.check_call(["make", "-s", f"-j{jobs}", "-C", csrc, "all"])


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run ngsld_amd.capi.build() (or make -C ngsld_amd/csrc); "
                                    "there is no fallback implementation")
        L = C.CDLL(LIB_PATH)
        vp, u64, dbl = C.c_void_p, C.c_uint64, C.c_double
        L.ngsld_version.restype = C.c_char_p
        L.ngsld_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.ngsld_destroy.argtypes = [vp]
        L.ngsld_destroy.restype = None
        L.ngsld_last_error.argtypes = [vp]
        L.ngsld_last_error.restype = C.c_char_p
        L.ngsld_set_geno_raw.argtypes = [vp, vp, u64, u64, C.c_int, C.c_int, C.c_int]
        L.ngsld_set_geno_raw_opts.argtypes = [vp, vp, u64, u64, C.POINTER(GenoOpts)]
        L.ngsld_set_geno_lkl.argtypes = [vp, vp, vp, u64, u64, C.c_int]
        L.ngsld_get_maf.argtypes = [vp, vp]
        L.ngsld_set_pos_dist.argtypes = [vp, vp]
        L.ngsld_plan.argtypes = [vp, C.POINTER(Params), C.POINTER(u64)]
        L.ngsld_plan_rows.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32))]
        L.ngsld_run.argtypes = [vp, u64, u64, SINK_FN, vp]
        L.ngsld_run_device.argtypes = [vp, u64, u64, vp, vp, vp]
        if hasattr(L, "ngsld_set_replay_source"):  # (absent only from older A/B builds loaded through NGSLD_LIB)
            L.ngsld_set_replay_source.argtypes = [vp, READ_FN, vp]
            if hasattr(L, "ngsld_set_replay_matrix"):
                L.ngsld_set_replay_matrix.argtypes = [vp, vp]
            L.ngsld_set_replay.argtypes = [vp, C.c_int]
            L.ngsld_replay_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        if hasattr(L, "ngsld_replay_info"):
            L.ngsld_set_exact_store.argtypes = [vp, C.c_int]
            L.ngsld_replay_info.argtypes = [vp, C.POINTER(ReplayStats)]
            L.ngsld_finish_device.argtypes = [vp]
        if hasattr(L, "ngsld_set_text_output"):  # (absent only from older A/B builds loaded through NGSLD_LIB)
            L.ngsld_set_text_output.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int]
        L.ngsld_last_kernel_time.argtypes = [vp, C.POINTER(dbl), C.POINTER(u64), C.POINTER(u64)]
        L.ngsld_set_tuning.argtypes = [vp, C.c_uint32, u64]
        if hasattr(L, "ngsld_pair_kernel"):
            L.ngsld_pair_kernel.argtypes = [vp]
            L.ngsld_pair_kernel.restype = C.c_char_p
        L.ngsld_selftest.argtypes = [vp]
        if hasattr(L, "ngsld_selftest_format"):
            L.ngsld_selftest_format.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.c_char_p, u64, vp, C.POINTER(C.c_int32)]
            L.ngsld_selftest_printed.argtypes = [vp, u64, vp, C.c_int32, C.c_int32, dbl, vp, vp, vp, vp]
        L.ngsld_window_ends.argtypes = [vp, u64, C.POINTER(Params), vp]
        L.ngsld_plan_slabs.argtypes = [vp, u64, C.POINTER(Params), u64, vp, u64, C.POINTER(u64)]
        L.ngsld_slab_sites_for_budget.argtypes = [u64, u64]
        L.ngsld_slab_sites_for_budget.restype = u64
        if hasattr(L, "ngsld_sites_for_budget"):  # (absent only from older A/B builds loaded through NGSLD_LIB)
            L.ngsld_sites_for_budget.argtypes = [u64, u64, C.c_int]
            L.ngsld_sites_for_budget.restype = u64
        L.ngsld_device_memory.argtypes = [C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.ngsld_run_streamed.argtypes = [C.c_int, u64, u64, vp, C.POINTER(Params), C.POINTER(GenoOpts), u64, READ_FN, vp,
                                         vp, SINK_FN, vp, C.POINTER(u64), C.POINTER(u64), C.c_char_p, C.c_size_t]
        if hasattr(L, "ngsld_run_multi"):
            L.ngsld_plan_parts.argtypes = [vp, u64, C.POINTER(Params), C.c_int, vp]
            L.ngsld_run_multi.argtypes = [C.POINTER(C.c_int), C.c_int, u64, u64, vp, C.POINTER(Params), C.POINTER(GenoOpts),
                                          vp, READ_FN, vp, vp, MULTI_SINK_FN, vp, C.POINTER(C.c_char_p), C.c_int,
                                          C.POINTER(u64), C.c_char_p, C.c_size_t]
        if hasattr(L, "ngsld_multi_last_distribution"):
            L.ngsld_multi_last_distribution.argtypes = []
        if hasattr(L, "ngsld_rccl_selftest"):
            L.ngsld_rccl_selftest.argtypes = [C.c_int, u64, C.c_char_p, C.c_size_t]
        L.ngsld_host_read_geno_bin_range.argtypes = [C.c_char_p, u64, u64, u64, vp, C.c_char_p, C.c_size_t]
        L.ngsld_host_set_threads.argtypes = [C.c_int]
        L.ngsld_host_set_threads.restype = None
        L.ngsld_host_read_pos.argtypes = [C.c_char_p, C.c_int, u64, C.POINTER(vp), C.c_char_p, C.c_size_t]
        L.ngsld_host_pos_dist.argtypes = [vp]
        L.ngsld_host_pos_dist.restype = C.POINTER(dbl)
        L.ngsld_host_label.argtypes = [vp, u64]
        L.ngsld_host_label.restype = C.c_char_p
        L.ngsld_host_free_pos.argtypes = [vp]
        L.ngsld_host_free_pos.restype = None
        L.ngsld_host_pos_slice.argtypes = [vp, u64, u64]
        L.ngsld_host_pos_slice.restype = vp
        L.ngsld_host_geno_size_ok.argtypes = [u64, u64, u64]
        L.ngsld_host_read_geno_bin.argtypes = [C.c_char_p, u64, u64, vp, C.c_char_p, C.c_size_t]
        L.ngsld_host_read_geno_text.argtypes = [C.c_char_p, C.c_int, C.c_int, u64, u64, vp, C.POINTER(C.c_int),
                                                C.c_char_p, C.c_size_t]
        L.ngsld_host_format_header.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
        L.ngsld_host_format_header.restype = C.c_size_t
        L.ngsld_host_format_pair.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, dbl, vp, vp, dbl, dbl]
        L.ngsld_host_format_pair.restype = C.c_size_t
        L.ngsld_host_format_double.argtypes = [C.c_char_p, C.c_size_t, dbl, C.c_int]
        L.ngsld_host_format_double.restype = C.c_size_t
        L.ngsld_host_write_batch.argtypes = [C.POINTER(Batch), vp, vp, vp, C.c_int, C.c_int]
        L.ngsld_host_replay_pair.argtypes = [vp, vp, u64, C.POINTER(GenoOpts), vp, vp, vp]
        if hasattr(L, "ngsld_host_gz_open"):
            L.ngsld_host_gz_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
            L.ngsld_host_gz_close.argtypes = [vp]
        if hasattr(L, "ngsld_prune"):
            L.ngsld_prune.argtypes = [vp, C.POINTER(PruneParams), C.POINTER(C.c_char_p), vp, C.POINTER(PruneStats)]
            L.ngsld_host_prune_graph.argtypes = [u64, vp, u64, vp, vp, vp, C.c_int, vp, C.POINTER(u64)]
            L.ngsld_host_prune_label.argtypes = [dbl, C.c_int, C.c_char, C.POINTER(C.c_int64)]
        if hasattr(L, "ngsld_decay"):
            L.ngsld_decay.argtypes = [vp, C.POINTER(DecayParams), C.POINTER(DecayStats)]
            L.ngsld_decay_bins.argtypes = [vp, u64, vp, vp, vp, C.POINTER(u64)]
            L.ngsld_host_decay_fit.argtypes = [u64, vp, vp, C.c_int, dbl, dbl, C.POINTER(DecayFitResult)]
        if hasattr(L, "ngsld_blocks"):
            L.ngsld_blocks.argtypes = [vp, C.POINTER(BlocksParams), C.POINTER(C.c_char_p), C.POINTER(BlocksStats)]
            L.ngsld_blocks_sites.argtypes = [vp, u64, vp, C.POINTER(u64)]
            L.ngsld_blocks_matrix.argtypes = [vp, C.c_int, vp, vp]
            L.ngsld_blocks_text.argtypes = [vp, C.c_int, TEXT_FN, vp, C.POINTER(BlocksStats)]
        if hasattr(L, "ngsld_site_ld"):
            L.ngsld_site_ld.argtypes = [vp, C.POINTER(SiteLdParams), C.POINTER(SiteLdStats)]
            L.ngsld_site_ld_get.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        if hasattr(L, "ngsld_clusters"):
            L.ngsld_clusters.argtypes = [vp, C.POINTER(ClustersParams), C.POINTER(ClustersStats)]
            L.ngsld_clusters_sites.argtypes = [vp, vp]
            L.ngsld_clusters_table.argtypes = [vp, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]
        if hasattr(L, "ngsld_grid"):
            L.ngsld_grid.argtypes = [vp, C.POINTER(GridParams), C.POINTER(C.c_char_p), C.POINTER(GridStats)]
            L.ngsld_grid_cells.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(u64)]
            L.ngsld_grid_chromosomes.argtypes = [vp, u64, C.POINTER(C.c_char_p), C.POINTER(u64)]
            L.ngsld_grid_get.argtypes = [vp, C.c_int, u64, vp, vp, vp, vp]
        if hasattr(L, "ngsld_linked_pairs"):
            L.ngsld_linked_pairs.argtypes = [vp, C.POINTER(LinkedParams), C.POINTER(C.c_char_p), LINKED_FN, vp, C.POINTER(LinkedStats)]
        if hasattr(L, "ngsld_analyze"):
            L.ngsld_analyze.argtypes = [vp, C.POINTER(Analysis), C.c_uint32, C.POINTER(AnalyzeStats)]
        if hasattr(L, "ngsld_scan"):
            L.ngsld_scan.argtypes = [vp, C.POINTER(ScanParams), C.POINTER(ScanStats)]
            L.ngsld_scan_get.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "ngsld_partners"):
            L.ngsld_partners.argtypes = [vp, C.POINTER(PartnersParams), vp, C.POINTER(PartnersStats)]
            L.ngsld_partners_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(C.c_uint32)]
            L.ngsld_partners_get.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "ngsld_decay_map"):
            L.ngsld_decay_map.argtypes = [vp, C.POINTER(DecayMapParams), C.POINTER(C.c_char_p), C.POINTER(DecayMapStats)]
            L.ngsld_decay_map_chromosomes.argtypes = [vp, u64, C.POINTER(C.c_char_p), C.POINTER(u64)]
            L.ngsld_decay_map_groups.argtypes = [vp, u64, vp, vp, vp, vp, C.POINTER(u64)]
            L.ngsld_decay_map_bins.argtypes = [vp, u64, vp, vp, vp, C.POINTER(u64)]
        if hasattr(L, "ngsld_cross_ld"):
            L.ngsld_cross_ld.argtypes = [vp, C.POINTER(CrossLdParams), C.POINTER(C.c_char_p), C.POINTER(CrossLdStats)]
            L.ngsld_cross_ld_cells.argtypes = [vp, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
            L.ngsld_cross_ld_chromosomes.argtypes = [vp, u64, C.POINTER(C.c_char_p), C.POINTER(u64)]
            L.ngsld_cross_ld_get.argtypes = [vp, C.c_int, u64, vp, vp, vp, vp]
        if hasattr(L, "ngsld_ld_tree"):
            L.ngsld_ld_tree.argtypes = [vp, C.POINTER(TreeParams), C.POINTER(TreeStats)]
            L.ngsld_ld_tree_merges.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]
            L.ngsld_ld_tree_cut.argtypes = [vp, C.c_double, vp, C.POINTER(u64)]
        _lib = L
    return _lib


def prune_label(x: float, prec: int = 4, weight_type: str = "a") -> int | None:
    """ngsld_host_prune_label: the edge label of one value as the pruner sees it printed; None for NaN / inf."""
    out = C.c_int64()
    rc = lib().ngsld_host_prune_label(float(x), prec, weight_type.encode(), C.byref(out))
    if rc == ERR_INVALID:
        return None
    if rc != OK:
        raise NgsldError(rc, "label out of range")
    return out.value


def decay_fit(dist, values, field: str = "r2", n_ind: float = 0, recomb_rate: float = 1.0) -> dict:
    """ngsld_host_decay_fit: the LD decay fit of fit_LDdecay.R on bin means (DECAY.md); field r2, r2_ExpG or Dp.  Returns
    {rate, ld_max, ld_min, sse, n_bins}; NgsldError for D, Dp with n_ind > 0, no bins or a bad value."""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    v = np.ascontiguousarray(values, dtype=np.float64)
    if d.shape != v.shape or d.ndim != 1:
        raise ValueError("dist and values must be 1-D arrays of one length")
    if field not in DECAY_FIELDS:
        raise ValueError(f"field must be one of {DECAY_FIELDS}")
    out = DecayFitResult()
    rc = lib().ngsld_host_decay_fit(len(d), d.ctypes.data, v.ctypes.data, 4 + DECAY_FIELDS.index(field), float(n_ind),
                                    float(recomb_rate), C.byref(out))
    if rc != OK:
        raise NgsldError(rc, f"ngsld_host_decay_fit refused the {field} fit")
    return {k: getattr(out, k) for k, _ in DecayFitResult._fields_}


def decay_map_fit(groups: list[dict], field: str = "r2", n_ind: float = 0, recomb_rate: float = 1.0, min_bins: int = 3) -> list:
    """decay_fit on each group of Engine.decay_map's list, in its order: the fit's dict, or None where the group has fewer than
    min_bins bins (3: the parameters of the fit)."""
    return [decay_fit(g["dist"], g[field], field, n_ind, recomb_rate) if len(g["dist"]) >= max(int(min_bins), 1) else None
            for g in groups]


def prune_graph(n_nodes: int, a, b, label, keep_heavy: bool = False, rank=None) -> tuple[np.ndarray, int]:
    """ngsld_host_prune_graph: the exact sequential pruner on an edge list; returns (excluded[n_nodes] bool, steps)."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    lab = np.ascontiguousarray(label, dtype=np.int64)
    rk = None if rank is None else np.ascontiguousarray(rank, dtype=np.uint64)
    excl = np.zeros(max(n_nodes, 1), dtype=np.uint8)
    steps = C.c_uint64()
    rc = lib().ngsld_host_prune_graph(n_nodes, None if rk is None else rk.ctypes.data, len(a), a.ctypes.data, b.ctypes.data,
                                      lab.ctypes.data, int(keep_heavy), excl.ctypes.data, C.byref(steps))
    if rc != OK:
        raise NgsldError(rc, "ngsld_host_prune_graph failed")
    return excl[:n_nodes].astype(bool), steps.value


# ------------------------------------------------------------------------------------------------
# host helpers (no device)
# ------------------------------------------------------------------------------------------------
def read_pos(path: str, header: bool, n_sites: int) -> tuple[np.ndarray, list[str]]:
    L = lib()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.ngsld_host_read_pos(path.encode(), int(header), n_sites, C.byref(h), err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    try:
        pd = np.ctypeslib.as_array(L.ngsld_host_pos_dist(h), shape=(n_sites,)).copy()
        labels = [L.ngsld_host_label(h, s).decode() for s in range(n_sites)]
    finally:
        L.ngsld_host_free_pos(h)
    return pd, labels


def read_geno_bin(path: str, n_ind: int, n_sites: int) -> np.ndarray:
    L = lib()
    out = np.empty((n_sites, n_ind, 3), dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = L.ngsld_host_read_geno_bin(path.encode(), n_ind, n_sites, out.ctypes.data, err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    return out


def read_geno_bin_range(path: str, n_ind: int, site_begin: int, n_sites: int) -> np.ndarray:
    L = lib()
    out = np.empty((n_sites, n_ind, 3), dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = L.ngsld_host_read_geno_bin_range(path.encode(), n_ind, site_begin, n_sites, out.ctypes.data, err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    return out


def _params(max_kb_dist=0, max_snp_dist=0, min_maf=0.0, ignore_miss_data=False, extend_out=True, rnd_sample=1.0, seed=0,
            first_row=0) -> Params:
    return Params(max_kb_dist, max_snp_dist, min_maf, int(ignore_miss_data), int(extend_out), rnd_sample, seed, first_row)


def window_ends(pos_dist: np.ndarray | None, n_sites: int, **kw) -> np.ndarray:
    """row_end[s1] from the distance / SNP-count limits alone (host only)."""
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    out = np.empty(n_sites, dtype=np.uint32)
    p = _params(**kw)
    rc = lib().ngsld_window_ends(None if pd is None else pd.ctypes.data, n_sites, C.byref(p), out.ctypes.data)
    if rc != OK:
        raise NgsldError(rc, "ngsld_window_ends")
    return out


def plan_slabs(pos_dist: np.ndarray | None, n_sites: int, max_slab_sites: int, **kw) -> np.ndarray:
    """Slabs (row_begin, row_end, site_end) of a streamed run (host only)."""
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    out = np.zeros(n_sites, dtype=SLAB)
    n = C.c_uint64()
    p = _params(**kw)
    rc = lib().ngsld_plan_slabs(None if pd is None else pd.ctypes.data, n_sites, C.byref(p), max_slab_sites,
                                out.ctypes.data, n_sites, C.byref(n))
    if rc != OK:
        raise NgsldError(rc, "the window of a single site does not fit the slab" if rc == ERR_NOMEM else "ngsld_plan_slabs")
    return out[:n.value].copy()


def slab_sites_for_budget(n_ind: int, budget_bytes: int) -> int:
    return int(lib().ngsld_slab_sites_for_budget(n_ind, budget_bytes))


def sites_for_budget(n_ind: int, budget_bytes: int, matrix_copies: int) -> int:
    """ngsld_sites_for_budget: the matrix priced matrix_copies times per context (1: the planes alone; 3: with the exact store)."""
    return int(lib().ngsld_sites_for_budget(n_ind, budget_bytes, matrix_copies))


def streamed_replay_info() -> dict:
    """ngsld_streamed_replay_info: where the flagged pairs of the last streamed job were replayed, summed over its slabs."""
    st = ReplayStats()
    L = lib()
    L.ngsld_streamed_replay_info.argtypes = [C.POINTER(ReplayStats)]
    rc = L.ngsld_streamed_replay_info(C.byref(st))
    if rc != OK:
        raise NgsldError(rc, "ngsld_streamed_replay_info")
    return {k: getattr(st, k) for k, _ in ReplayStats._fields_}


def set_memory_budget(device: int, n_bytes: int) -> None:
    """ngsld_set_memory_budget: a cap on what this process takes of the device's memory from now on (0: none)."""
    L = lib()
    L.ngsld_set_memory_budget.argtypes = [C.c_int, C.c_uint64]
    rc = L.ngsld_set_memory_budget(device, n_bytes)
    if rc != OK:
        raise NgsldError(rc, "ngsld_set_memory_budget")


def device_memory(device: int = 0) -> tuple[int, int]:
    f, t = C.c_uint64(), C.c_uint64()
    rc = lib().ngsld_device_memory(device, C.byref(f), C.byref(t))
    if rc != OK:
        raise NgsldError(rc, "ngsld_device_memory")
    return f.value, t.value


def run_streamed(read_sites, n_sites: int, n_ind: int, pos_dist: np.ndarray | None, max_slab_sites: int, device: int = 0,
                 log_scale: bool = False, call_geno: tuple[float, float] | None = None, text: bool = False, **kw):
    """The whole job slab by slab (ngsld_run_streamed).  read_sites(site_begin, n) -> array [n, n_ind, 3] of raw values.
    Returns (s1, s2, std, ext, maf, n_slabs) with global site indices."""
    L = lib()
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    p = _params(**kw)
    o = GenoOpts(int(log_scale), p.ignore_miss_data, 0, int(text), int(call_geno is not None), 0,
                 call_geno[0] if call_geno else 0.0, call_geno[1] if call_geno else 0.0)
    s1s, s2s, stds, exts = [], [], [], []

    def reader(_user, site_begin, n, dst):
        try:
            a = np.ascontiguousarray(read_sites(int(site_begin), int(n)), dtype=np.float64)
            assert a.size == n * n_ind * 3
            C.memmove(dst, a.ctypes.data, a.nbytes)
            return 0
        except Exception:  # noqa: BLE001 -- reported through the return code
            return 1

    def sink(_user, bp):
        b = bp.contents
        n = b.n_pairs
        if n:
            stds.append(np.frombuffer(C.string_at(b.std, n * REC_STD.itemsize), dtype=REC_STD).copy())
            if b.ext:
                exts.append(np.frombuffer(C.string_at(b.ext, n * REC_EXT.itemsize), dtype=REC_EXT).copy())
        items = np.frombuffer(C.string_at(b.items, b.n_items * ITEM.itemsize), dtype=ITEM) if b.n_items else \
            np.zeros(0, dtype=ITEM)
        a, bb = items_to_pairs(items)
        assert len(a) == n and (n == 0 or (a.min() >= b.s1_begin and a.max() < b.s1_end))
        s1s.append(a)
        s2s.append(bb)
        return 0

    maf = np.full(n_sites, np.nan)
    n_pairs, n_slabs = C.c_uint64(), C.c_uint64()
    err = C.create_string_buffer(512)
    rcb, scb = READ_FN(reader), SINK_FN(sink)
    rc = L.ngsld_run_streamed(device, n_sites, n_ind, None if pd is None else pd.ctypes.data, C.byref(p), C.byref(o),
                              max_slab_sites, rcb, None, maf.ctypes.data, scb, None, C.byref(n_pairs), C.byref(n_slabs),
                              err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    s1 = cat(s1s, np.uint64)
    assert len(s1) == n_pairs.value
    return (s1, cat(s2s, np.uint64), cat(stds, REC_STD), cat(exts, REC_EXT) if p.extend_out else None, maf,
            int(n_slabs.value))


def plan_parts(pos_dist: np.ndarray | None, n_sites: int, n_parts: int, **kw) -> np.ndarray:
    """Row parts (row_begin, row_end, site_end) of a multi-device run (host only)."""
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    out = np.zeros(n_parts, dtype=SLAB)
    p = _params(**kw)
    rc = lib().ngsld_plan_parts(None if pd is None else pd.ctypes.data, n_sites, C.byref(p), n_parts, out.ctypes.data)
    if rc != OK:
        raise NgsldError(rc, "ngsld_plan_parts")
    return out


def run_multi(raw: np.ndarray, pos_dist: np.ndarray | None, devices: list[int], log_scale: bool = False,
              call_geno: tuple[float, float] | None = None, text: bool = False, labels: list[str] | None = None,
              text_output: bool = False, **kw):
    """One job over several devices in this process (ngsld_run_multi).  Returns per part a tuple
    (s1, s2, std, ext) -- or the part's TSV bytes with text_output -- plus the maf vector and the pairs per part."""
    L = lib()
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    n_sites, n_ind = raw.shape[0], raw.shape[1]
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    p = _params(**kw)
    o = GenoOpts(int(log_scale), p.ignore_miss_data, 0, int(text), int(call_geno is not None), 0,
                 call_geno[0] if call_geno else 0.0, call_geno[1] if call_geno else 0.0)
    n = len(devices)
    acc = [dict(s1=[], s2=[], std=[], ext=[], text=[]) for _ in range(n)]

    def sink(_user, part, bp):
        b = bp.contents
        a = acc[part]
        if b.text:
            a["text"].append(C.string_at(b.text, b.text_len))
            return 0
        k = b.n_pairs
        if k:
            a["std"].append(np.frombuffer(C.string_at(b.std, k * REC_STD.itemsize), dtype=REC_STD).copy())
            if b.ext:
                a["ext"].append(np.frombuffer(C.string_at(b.ext, k * REC_EXT.itemsize), dtype=REC_EXT).copy())
        items = np.frombuffer(C.string_at(b.items, b.n_items * ITEM.itemsize), dtype=ITEM) if b.n_items else \
            np.zeros(0, dtype=ITEM)
        x, y = items_to_pairs(items)
        a["s1"].append(x)
        a["s2"].append(y)
        return 0

    maf = np.full(n_sites, np.nan)
    per = (C.c_uint64 * n)()
    err = C.create_string_buffer(512)
    devs = (C.c_int * n)(*devices)
    lab = None
    if labels is not None:
        lab = (C.c_char_p * len(labels))(*[l.encode() for l in labels])
    cb = MULTI_SINK_FN(sink)
    rc = L.ngsld_run_multi(devs, n, n_sites, n_ind, None if pd is None else pd.ctypes.data, C.byref(p), C.byref(o),
                           raw.ctypes.data, READ_FN(0), None, maf.ctypes.data, cb, None, lab, int(text_output), per, err,
                           len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    out = []
    for a in acc:
        if text_output:
            out.append(b"".join(a["text"]))
        else:
            out.append((cat(a["s1"], np.uint64), cat(a["s2"], np.uint64), cat(a["std"], REC_STD),
                        cat(a["ext"], REC_EXT) if p.extend_out else None))
    return out, maf, [int(v) for v in per]


def run_multi_sink(raw: np.ndarray, pos_dist: np.ndarray | None, devices: list[int], sink=None, log_scale: bool = False, **kw):
    """ngsld_run_multi with the records left where they arrive: sink(part, n_pairs, std, ext) sees every batch as numpy
    views of the library's host buffers (valid during the call; called on the part's own thread), or nothing is looked at
    when sink is None.  Returns the pairs per part."""
    L = lib()
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    n_sites, n_ind = raw.shape[0], raw.shape[1]
    pd = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64)
    p = _params(**kw)
    o = GenoOpts(int(log_scale), p.ignore_miss_data, 0, 0, 0, 0, 0.0, 0.0)
    n = len(devices)

    def cb(_user, part, bp):
        if sink is None:
            return 0
        b = bp.contents
        k = b.n_pairs
        if k == 0:
            return 0
        std = np.ctypeslib.as_array(C.cast(b.std, C.POINTER(C.c_uint8)), shape=(k * REC_STD.itemsize,)).view(REC_STD)
        ext = np.ctypeslib.as_array(C.cast(b.ext, C.POINTER(C.c_uint8)), shape=(k * REC_EXT.itemsize,)).view(REC_EXT) \
            if b.ext else None
        return int(sink(part, k, std, ext) or 0)

    per = (C.c_uint64 * n)()
    err = C.create_string_buffer(512)
    devs = (C.c_int * n)(*devices)
    rc = L.ngsld_run_multi(devs, n, n_sites, n_ind, None if pd is None else pd.ctypes.data, C.byref(p), C.byref(o),
                           raw.ctypes.data, READ_FN(0), None, None, MULTI_SINK_FN(cb), None, None, 0, per, err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    return [int(v) for v in per]


DIST_NAMES = {0: "none", 1: "upload", 2: "peer_copy", 3: "rccl"}


def multi_last_distribution() -> str:
    """How the last run_multi of this process handed the matrix to its devices: "upload" (slab by slab), "peer_copy"
    (device to device from the first) or "rccl" (one ncclBroadcast over xGMI)."""
    return DIST_NAMES[int(lib().ngsld_multi_last_distribution())]


def rccl_selftest(device: int = 0, n_bytes: int = 64 << 20) -> None:
    """librccl's part in ngsld_run_multi on a one-device communicator (ngsld_rccl_selftest); raises NgsldError."""
    err = C.create_string_buffer(512)
    rc = lib().ngsld_rccl_selftest(device, n_bytes, err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())


def describe_dispatch(n_ind: int, ignore_miss_data: bool = False) -> str:
    """Kernel family and shape a likelihood matrix of n_ind individuals runs on (no device needed): ngsld_describe_dispatch."""
    buf = C.create_string_buffer(96)
    L = lib()
    L.ngsld_describe_dispatch.argtypes = [C.c_uint64, C.c_int, C.c_char_p, C.c_size_t]
    rc = L.ngsld_describe_dispatch(int(n_ind), int(bool(ignore_miss_data)), buf, 96)
    if rc != OK:
        raise NgsldError(rc, f"no kernel for n_ind = {n_ind}")
    return buf.value.decode()


def dispatch_table(n_max: int = 12_000) -> str:
    """describe_dispatch over 1..n_max for both settings of ignore_miss_data, as ranges of equal text."""
    import re
    lines = []

    def describe(n, masked):  # (the streaming kernel pads to the next 64 whatever the size: one line for all of them)
        d = describe_dispatch(n, masked)
        return re.sub(r"np=\d+", "np=n_ind rounded up to 64", d) if d.startswith("stream") else d

    for masked in (False, True):
        lines.append(f"# ignore_miss_data = {int(masked)}")
        lo, cur = 1, describe(1, masked)
        for n in range(2, n_max + 2):
            d = describe(n, masked) if n <= n_max else None
            if d != cur:
                lines.append(f"{lo}..{n - 1}\t{cur}")
                lo, cur = n, d
    return "\n".join(lines) + "\n"


def device_count() -> int:
    """GPUs visible to this process (hipGetDeviceCount through the library's own runtime; 0 without a GPU)."""
    n = 0
    while n < 64:
        free, total = C.c_uint64(0), C.c_uint64(0)
        if lib().ngsld_device_memory(n, C.byref(free), C.byref(total)) != OK:
            break
        n += 1
    return n


def read_geno_text(path: str, in_probs: bool, log_scale: bool, n_ind: int, n_sites: int) -> tuple[np.ndarray, bool]:
    """Text/.gz genotype file -> (raw [n_sites, n_ind, 3], values_are_logs) for Engine.set_geno_raw(text=True)."""
    L = lib()
    out = np.empty((n_sites, n_ind, 3), dtype=np.float64)
    err = C.create_string_buffer(512)
    is_log = C.c_int(0)
    rc = L.ngsld_host_read_geno_text(path.encode(), int(in_probs), int(log_scale), n_ind, n_sites, out.ctypes.data,
                                     C.byref(is_log), err, len(err))
    if rc != OK:
        raise NgsldError(rc, err.value.decode())
    return out, bool(is_log.value)


def replay_pair(raw1: np.ndarray, raw2: np.ndarray, log_scale: bool = False, ignore_miss_data: bool = False,
                text: bool = False, call_geno: tuple | None = None):
    """One pair in the reference's own operation order on the host (ngsld_host_replay_pair).
    raw1, raw2: [n_ind, 3] raw values of the two sites.  Returns (std record, ext record, (maf1, maf2))."""
    a = np.ascontiguousarray(raw1, dtype=np.float64)
    b = np.ascontiguousarray(raw2, dtype=np.float64)
    o = GenoOpts(int(log_scale), int(ignore_miss_data), 0, int(text), int(call_geno is not None), 0,
                 float(call_geno[0]) if call_geno else 0.0, float(call_geno[1]) if call_geno else 0.0)
    s, e, m = np.zeros(1, dtype=REC_STD), np.zeros(1, dtype=REC_EXT), np.zeros(2)
    rc = lib().ngsld_host_replay_pair(a.ctypes.data, b.ctypes.data, a.shape[0], C.byref(o), s.ctypes.data, e.ctypes.data,
                                      m.ctypes.data)
    if rc not in (OK, ERR_MAF_RANGE):
        raise NgsldError(rc, "ngsld_host_replay_pair")
    return s[0], e[0], (float(m[0]), float(m[1]))


def format_double(v: float, decimals: int = 6) -> str:
    buf = C.create_string_buffer(512)
    n = lib().ngsld_host_format_double(buf, len(buf), v, decimals)
    return buf.raw[:n].decode()


def format_header(extend_out: bool) -> str:
    buf = C.create_string_buffer(512)
    n = lib().ngsld_host_format_header(buf, len(buf), int(extend_out))
    return buf.raw[:n].decode()


def missing_call_log() -> float:
    """log(1/3) as the text reader stores it for a missing call (ngsld_host_missing_call_log)."""
    f = lib().ngsld_host_missing_call_log
    f.restype = C.c_double
    f.argtypes = []
    return float(f())


def format_pair(l1, l2, dist: float, std_rec: np.ndarray, ext_rec: np.ndarray | None, maf1: float, maf2: float) -> str:
    buf = C.create_string_buffer(8192)
    s = np.ascontiguousarray(std_rec).reshape(1).view(REC_STD) if std_rec.dtype != REC_STD else std_rec.reshape(1)
    e_ptr = None
    if ext_rec is not None:
        e = ext_rec.reshape(1)
        e_ptr = e.ctypes.data
    n = lib().ngsld_host_format_pair(buf, len(buf), None if l1 is None else l1.encode(),
                                     None if l2 is None else l2.encode(), dist, s.ctypes.data, e_ptr, maf1, maf2)
    return buf.raw[:n].decode()


# ------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------
class Engine:
    """One ngsld_ctx.  Mirrors the call order of the reference's main(): data -> positions -> run."""

    def __init__(self, device: int = 0):
        self._L = lib()
        self._h = C.c_void_p()
        rc = self._L.ngsld_create(device, C.byref(self._h))
        if rc != OK:
            raise NgsldError(rc, self._L.ngsld_last_error(None).decode())
        self.n_sites = self.n_ind = 0
        self.extend_out = False
        self._source = None

    def close(self) -> None:
        if self._h:
            self._L.ngsld_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != OK:
            raise NgsldError(rc, self._L.ngsld_last_error(self._h).decode())

    def selftest(self) -> None:
        self._check(self._L.ngsld_selftest(self._h))

    def selftest_format(self, std_rec: np.ndarray, ext_rec: np.ndarray | None, dist, maf1, maf2) -> tuple[list[str], bool]:
        """The device's TSV rows of n records (ngsld_selftest_format): row i the pair of sites (2i, 2i+1) with labels "(null)",
        dist[i] as its dist column (inf: a chromosome change) and maf1[i], maf2[i].  Returns (rows, needs_host)."""
        std_rec = np.ascontiguousarray(std_rec, dtype=REC_STD)
        n = len(std_rec)
        ext = None if ext_rec is None else np.ascontiguousarray(ext_rec, dtype=REC_EXT)
        assert ext is None or len(ext) == n
        d, m1, m2 = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (dist, maf1, maf2))
        cap = n * (400 if ext is None else 1200)
        text = C.create_string_buffer(cap)
        lens = np.zeros(n, dtype=np.uint64)
        host = C.c_int32()
        self._check(self._L.ngsld_selftest_format(self._h, n, std_rec.ctypes.data, None if ext is None else ext.ctypes.data,
                                                  d.ctypes.data, m1.ctypes.data, m2.ctypes.data, text, cap, lens.ctypes.data,
                                                  C.byref(host)))
        raw = text.raw[:int(lens.sum())].decode()
        ends = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return [raw[ends[i]:ends[i + 1]] for i in range(n)], bool(host.value)

    def selftest_printed(self, x, precision: int = 4, weight_type: str = "a", min_weight: float = 0.0) -> dict:
        """The device's printed-value quantiser (ngsld_selftest_printed) on the doubles x: arrays "micro" / "micro_ok" (LD
        decay's integer micro-units) and "label" / "rc" (LD pruning's edge label: rc 0 an edge, 1 skipped, 2 too large)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = len(x)
        out = {"micro": np.zeros(n, dtype=np.int64), "micro_ok": np.zeros(n, dtype=np.int32), "label": np.zeros(n, dtype=np.int64),
               "rc": np.zeros(n, dtype=np.int32)}
        self._check(self._L.ngsld_selftest_printed(self._h, n, x.ctypes.data, precision, ord(weight_type), float(min_weight),
                                                   out["micro"].ctypes.data, out["micro_ok"].ctypes.data,
                                                   out["label"].ctypes.data, out["rc"].ctypes.data))
        return out

    def set_geno_raw(self, gl, n_sites: int | None = None, n_ind: int | None = None, log_scale: bool = False,
                     ignore_miss_data: bool = False, text: bool = False, call_geno: tuple | None = None,
                     per_individual_only: bool = False, replay_source: bool = True) -> None:
        """gl: numpy float64 [n_sites, n_ind, 3] (host) or an int device pointer with explicit sizes.
        text: values come from a text genotype file (read_geno_text); call_geno = (N_thresh, call_thresh)."""
        if isinstance(gl, np.ndarray):
            gl = np.ascontiguousarray(gl, dtype=np.float64)
            n_sites, n_ind = gl.shape[0], gl.shape[1]
            ptr, on_dev = gl.ctypes.data, 0
        else:
            ptr, on_dev = int(gl), 1
        o = GenoOpts(int(log_scale), int(ignore_miss_data), on_dev, int(text), int(call_geno is not None), int(per_individual_only),
                     float(call_geno[0]) if call_geno else 0.0, float(call_geno[1]) if call_geno else 0.0)
        self._check(self._L.ngsld_set_geno_raw_opts(self._h, ptr, n_sites, n_ind, C.byref(o)))
        self.n_sites, self.n_ind = n_sites, n_ind
        self._source = None
        if isinstance(gl, np.ndarray) and replay_source:
            self.set_replay_source(gl)

    def set_geno_lkl(self, geno_lkl: np.ndarray, maf: np.ndarray, replay_source: bool = True) -> None:
        g = np.ascontiguousarray(geno_lkl, dtype=np.float64)
        m = np.ascontiguousarray(maf, dtype=np.float64)
        self._check(self._L.ngsld_set_geno_lkl(self._h, g.ctypes.data, m.ctypes.data, g.shape[0], g.shape[1], 0))
        self.n_sites, self.n_ind = g.shape[0], g.shape[1]
        self._source = None
        if replay_source:
            self.set_replay_source(g)

    def set_replay_source(self, values: np.ndarray | None) -> None:
        """The matrix the exact-order replay reads the flagged pairs' sites from again: the array given to set_geno_raw /
        set_geno_lkl (kept alive by this object).  None: the library reads its own planes back from the device."""
        if values is None or not hasattr(self._L, "ngsld_set_replay_source"):
            self._source = None
            if hasattr(self._L, "ngsld_set_replay_source"):
                self._check(self._L.ngsld_set_replay_source(self._h, READ_FN(0), None))
            return
        arr = np.ascontiguousarray(values, dtype=np.float64).reshape(self.n_sites, -1)
        row = arr.shape[1] * 8
        if hasattr(self._L, "ngsld_set_replay_matrix") and os.environ.get("NGSLD_PY_REPLAY_CALLBACK") != "1":
            self._source = (arr, None)   # read in place by the library's replay threads: no callback, no GIL
            self._check(self._L.ngsld_set_replay_matrix(self._h, arr.ctypes.data))
            return

        def reader(_user, site_begin, n, dst):
            if site_begin + n > arr.shape[0]:
                return 1
            C.memmove(dst, arr.ctypes.data + int(site_begin) * row, int(n) * row)
            return 0

        cb = READ_FN(reader)
        self._source = (arr, cb)
        self._check(self._L.ngsld_set_replay_source(self._h, cb, None))

    def set_replay(self, enable: bool) -> None:
        self._check(self._L.ngsld_set_replay(self._h, int(enable)))

    def replay_stats(self) -> tuple[int, int]:
        """(pairs replayed by the last run, sites re-evaluated by the last plan + run)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.ngsld_replay_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_exact_store(self, mode: int) -> None:
        """0: flagged pairs of a likelihood matrix are replayed on host threads only; 1 (default): on the device once a run
        flags more of them than the host should replay; 2: from the first flagged pair on (ngsld_set_exact_store)."""
        self._check(self._L.ngsld_set_exact_store(self._h, int(mode)))

    def replay_info(self) -> dict:
        """ngsld_replay_info: where the flagged pairs of the last run were replayed."""
        st = ReplayStats()
        self._check(self._L.ngsld_replay_info(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in ReplayStats._fields_}

    def finish_device(self) -> None:
        self._check(self._L.ngsld_finish_device(self._h))

    def maf(self) -> np.ndarray:
        out = np.empty(self.n_sites, dtype=np.float64)
        self._check(self._L.ngsld_get_maf(self._h, out.ctypes.data))
        return out

    def set_pos_dist(self, pos_dist: np.ndarray | None) -> None:
        if pos_dist is None:
            self._check(self._L.ngsld_set_pos_dist(self._h, None))
        else:
            pd = np.ascontiguousarray(pos_dist, dtype=np.float64)
            assert pd.shape[0] == self.n_sites
            self._check(self._L.ngsld_set_pos_dist(self._h, pd.ctypes.data))

    def set_tuning(self, pairs_per_item: int = 0, batch_pairs: int = 0) -> None:
        self._check(self._L.ngsld_set_tuning(self._h, pairs_per_item, batch_pairs))

    def plan(self, max_kb_dist: int = 0, max_snp_dist: int = 0, min_maf: float = 0.0, ignore_miss_data: bool = False,
             extend_out: bool = True, rnd_sample: float = 1.0, seed: int = 0, first_row: int = 0) -> int:
        p = Params(max_kb_dist, max_snp_dist, min_maf, int(ignore_miss_data), int(extend_out), rnd_sample, seed,
                   first_row)
        n = C.c_uint64()
        self._check(self._L.ngsld_plan(self._h, C.byref(p), C.byref(n)))
        self.extend_out = extend_out
        return n.value

    def plan_rows(self) -> tuple[np.ndarray, np.ndarray]:
        ro, re = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
        self._check(self._L.ngsld_plan_rows(self._h, C.byref(ro), C.byref(re)))
        return (np.ctypeslib.as_array(ro, shape=(self.n_sites + 1,)).copy(),
                np.ctypeslib.as_array(re, shape=(self.n_sites,)).copy())

    def run(self, s1_begin: int = 0, s1_end: int | None = None):
        """Run rows [s1_begin, s1_end) through the sink path; returns (s1, s2, std, ext) arrays."""
        s1_end = self.n_sites if s1_end is None else s1_end
        s1s, s2s, stds, exts = [], [], [], []

        def sink(_user, bp):
            b = bp.contents
            n = b.n_pairs
            if n:
                stds.append(np.frombuffer(C.string_at(b.std, n * REC_STD.itemsize), dtype=REC_STD).copy())
                if b.ext:
                    exts.append(np.frombuffer(C.string_at(b.ext, n * REC_EXT.itemsize), dtype=REC_EXT).copy())
            items = np.frombuffer(C.string_at(b.items, b.n_items * ITEM.itemsize), dtype=ITEM) if b.n_items else \
                np.zeros(0, dtype=ITEM)
            a, bb = items_to_pairs(items)
            assert len(a) == n
            if len(items):
                assert np.array_equal(items["first_record"], np.concatenate([[0], np.cumsum(
                    [bin(int(m)).count("1") for m in items["mask"]])[:-1]]).astype(np.uint64))
            s1s.append(a)
            s2s.append(bb)
            return 0

        cb = SINK_FN(sink)
        self._check(self._L.ngsld_run(self._h, s1_begin, s1_end, cb, None))
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
        return (cat(s1s, np.uint64), cat(s2s, np.uint64), cat(stds, REC_STD),
                cat(exts, REC_EXT) if self.extend_out else None)

    def items(self, s1_begin: int = 0, s1_end: int | None = None) -> np.ndarray:
        """The work items (dtype ITEM) of rows [s1_begin, s1_end), as a record run's batches hand them to the sink; leaves
        device-side text output off."""
        s1_end = self.n_sites if s1_end is None else s1_end
        got = []

        def sink(_user, bp):
            b = bp.contents
            if b.n_items:
                got.append(np.frombuffer(C.string_at(b.items, b.n_items * ITEM.itemsize), dtype=ITEM).copy())
            return 0

        self.set_text_output(None, False)
        self._check(self._L.ngsld_run(self._h, s1_begin, s1_end, SINK_FN(sink), None))
        return np.concatenate(got) if got else np.zeros(0, dtype=ITEM)

    def run_to_fd(self, s1_begin: int, s1_end: int, fd: int, pos_handle, pos_dist: np.ndarray | None, maf: np.ndarray,
                  n_threads: int) -> int:
        """Rows [s1_begin, s1_end) -> TSV rows on file descriptor fd: text batches (after set_text_output) are written
        as they come, record batches go through ngsld_host_write_batch."""
        maf = np.ascontiguousarray(maf, dtype=np.float64)
        pd_ptr = None if pos_dist is None else np.ascontiguousarray(pos_dist, dtype=np.float64).ctypes.data
        total, rc_box = [0], [0]

        libc = C.CDLL(None, use_errno=True)
        libc.write.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
        libc.write.restype = C.c_ssize_t

        def sink(_user, bp):
            b = bp.contents
            total[0] += b.n_pairs
            if b.text:                                   # rows formatted on the device (set_text_output): only bytes to write
                off = 0
                while off < b.text_len:
                    w = libc.write(fd, b.text + off, min(b.text_len - off, 1 << 30))
                    if w <= 0:
                        return 1
                    off += w
                return 0
            rc_box[0] = self._L.ngsld_host_write_batch(bp, pos_handle, pd_ptr, maf.ctypes.data, n_threads, fd)
            return 0 if rc_box[0] == OK else 1

        self._check(self._L.ngsld_run(self._h, s1_begin, s1_end, SINK_FN(sink), None))
        return total[0]

    def set_text_output(self, labels: list[str] | None, enable: bool = True) -> None:
        """Device-side TSV: ngsld_run then hands over text instead of records (labels None = "(null)")."""
        arr = None
        if labels is not None:
            arr = (C.c_char_p * len(labels))(*[l.encode() for l in labels])
        self._check(self._L.ngsld_set_text_output(self._h, arr, int(enable)))

    def run_text(self, s1_begin: int = 0, s1_end: int | None = None) -> tuple[bytes, int]:
        """Run through the sink path with device-side TSV on; returns (text of all batches, batches that arrived
        as records instead)."""
        s1_end = self.n_sites if s1_end is None else s1_end
        parts, fallbacks = [], [0]

        def sink(_user, bp):
            b = bp.contents
            if b.text:
                parts.append(C.string_at(b.text, b.text_len))
            else:
                fallbacks[0] += 1
            return 0

        self._check(self._L.ngsld_run(self._h, s1_begin, s1_end, SINK_FN(sink), None))
        return b"".join(parts), fallbacks[0]

    def run_discard(self, s1_begin: int = 0, s1_end: int | None = None) -> int:
        """Run through the sink path (kernel + D2H of every record into pinned host memory) and only count the
        pairs delivered: the host-buffer hand-off rate without any formatting."""
        s1_end = self.n_sites if s1_end is None else s1_end
        total = [0]

        def sink(_user, bp):
            total[0] += bp.contents.n_pairs
            return 0

        self._check(self._L.ngsld_run(self._h, s1_begin, s1_end, SINK_FN(sink), None))
        return total[0]

    def run_device(self, s1_begin: int, s1_end: int, d_std: int, d_ext: int | None, stream: int | None = None) -> None:
        self._check(self._L.ngsld_run_device(self._h, s1_begin, s1_end, d_std, d_ext, stream))

    def pair_kernel(self) -> str:
        """Kernel family of the data set last: group / run / wave / multi / stream / direct / hard."""
        return self._L.ngsld_pair_kernel(self._h).decode()

    def last_kernel_time(self) -> tuple[float, int, int]:
        ms, nl, npairs = C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self._L.ngsld_last_kernel_time(self._h, C.byref(ms), C.byref(nl), C.byref(npairs)))
        return ms.value, nl.value, npairs.value

    def prune(self, labels: list[str] | None, field: int = 7, max_kb_dist: float = float("inf"), min_weight: float = 0.0,
              weight_type: str = "a", keep_heavy: bool = False, subset: list[str] | None = None,
              precision: int = 4) -> tuple[np.ndarray, dict]:
        """LD pruning of the planned pairs on the device (ngsld_prune): (site_state, stats) -- site_state[s] is 0 (not a node),
        1 (kept) or 2 (excluded); labels None = every label "(null)"."""
        return self._prune_job(labels, field, max_kb_dist, min_weight, weight_type, keep_heavy, subset, precision).run()

    def _prune_job(self, labels: list[str] | None, field: int = 7, max_kb_dist: float = float("inf"), min_weight: float = 0.0,
                   weight_type: str = "a", keep_heavy: bool = False, subset: list[str] | None = None,
                   precision: int = 4) -> _Job:
        arr = None if labels is None else (C.c_char_p * len(labels))(*[l.encode() for l in labels])
        sub = None if subset is None else (C.c_char_p * max(len(subset), 1))(*[l.encode() for l in subset])
        p = PruneParams(C.sizeof(PruneParams), field, float(max_kb_dist), float(min_weight), ord(weight_type), int(keep_heavy),
                        precision, 0, sub, 0 if subset is None else len(subset))
        st = PruneStats()
        st.struct_size = C.sizeof(PruneStats)
        state = np.zeros(max(self.n_sites, 1), dtype=np.uint8)

        def call():
            self._check(self._L.ngsld_prune(self._h, C.byref(p), arr, state.ctypes.data, C.byref(st)))

        def read():
            return state[:self.n_sites], {k: getattr(st, k) for k, _ in PruneStats._fields_ if k not in ("struct_size", "reserved")}

        job = _Job(AN_PRUNE, p, st, call, read, labels=arr, site_state=state)
        job.keep = sub  # (the params point into it)
        return job

    def decay(self, ld=("r2",), bin_size: float = 250, max_kb_dist: float = float("inf"),
              min_maf: float = 0.0) -> tuple[dict, dict]:
        """LD decay bins of the planned pairs on the device (ngsld_decay): (bins, stats).  bins holds numpy arrays "dist" (each
        non-empty bin's lower break), "n" (rows) and one mean per statistic of ld (r2_ExpG, D, Dp, r2)."""
        return self._decay_job(ld, bin_size, max_kb_dist, min_maf).run()

    def _decay_job(self, ld=("r2",), bin_size: float = 250, max_kb_dist: float = float("inf"), min_maf: float = 0.0) -> _Job:
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        names = [f for k, f in enumerate(DECAY_FIELDS) if (mask >> k) & 1]
        p = DecayParams(C.sizeof(DecayParams), mask, float(bin_size), float(max_kb_dist), float(min_maf))
        st = DecayStats()
        st.struct_size = C.sizeof(DecayStats)

        def call():
            self._check(self._L.ngsld_decay(self._h, C.byref(p), C.byref(st)))

        return _Job(AN_DECAY, p, st, call, lambda: self._decay_read(st, names))

    def _decay_read(self, st, names) -> tuple[dict, dict]:
        nb = st.bins
        dist = np.zeros(max(nb, 1))
        cnt = np.zeros(max(nb, 1), dtype=np.uint64)
        mean = np.zeros((max(nb, 1), len(names)))
        got = C.c_uint64()
        self._check(self._L.ngsld_decay_bins(self._h, nb, dist.ctypes.data, cnt.ctypes.data, mean.ctypes.data, C.byref(got)))
        assert got.value == nb
        return self._bin_columns(dist, cnt, mean, names, 0, nb), {k: getattr(st, k) for k, _ in DecayStats._fields_ if k != "struct_size"}

    @staticmethod
    def _bin_columns(dist, cnt, mean, names, a, b) -> dict:
        """Bins a .. b - 1 of the arrays of ngsld_decay_bins / ngsld_decay_map_bins: one group's "dist", "n" and a mean per statistic."""
        bins = {"dist": dist[a:b].copy(), "n": cnt[a:b].copy()}
        for k, f in enumerate(names):
            bins[f] = mean[a:b, k].copy()
        return bins

    def decay_map(self, labels: list[str] | None, window: int = 0, ld=("r2",), bin_size: float = 250,
                  max_kb_dist: float = float("inf"), min_maf: float = 0.0) -> tuple[list, dict]:
        """The LD decay map of the planned pairs on the device (ngsld_decay_map, DECAY_MAP.md): (groups, stats).  A group is a
        chromosome (window 0; labels may be None, the groups are then named "1", "2", ...) or the window of `window` bp that
        holds a pair's midpoint.  groups lists, in result order, {"chr", "win_start", "dist", "n", <one array per statistic>}:
        the arrays are those Engine.decay returns for a table of that group's rows alone."""
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        names = [f for k, f in enumerate(DECAY_FIELDS) if (mask >> k) & 1]
        arr = None if labels is None else (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels])
        p = DecayMapParams(C.sizeof(DecayMapParams), mask, float(bin_size), float(max_kb_dist), float(min_maf), int(window))
        st = DecayMapStats()
        st.struct_size = C.sizeof(DecayMapStats)
        self._check(self._L.ngsld_decay_map(self._h, C.byref(p), arr, C.byref(st)))
        return self._decay_map_read(names), {k: getattr(st, k) for k, _ in DecayMapStats._fields_ if k != "struct_size"}

    def _decay_map_read(self, names) -> list:
        n_chr, ng, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.ngsld_decay_map_chromosomes(self._h, 0, None, C.byref(n_chr)))
        chr_name = (C.c_char_p * max(int(n_chr.value), 1))()
        self._check(self._L.ngsld_decay_map_chromosomes(self._h, int(n_chr.value), chr_name, None))
        self._check(self._L.ngsld_decay_map_groups(self._h, 0, None, None, None, None, C.byref(ng)))
        self._check(self._L.ngsld_decay_map_bins(self._h, 0, None, None, None, C.byref(nb)))
        ng, nb = int(ng.value), int(nb.value)
        idx = np.zeros(max(ng, 1), dtype=np.uint32)
        win, first, length = (np.zeros(max(ng, 1), dtype=np.uint64) for _ in range(3))
        dist, cnt = np.zeros(max(nb, 1)), np.zeros(max(nb, 1), dtype=np.uint64)
        mean = np.zeros((max(nb, 1), len(names)))
        self._check(self._L.ngsld_decay_map_groups(self._h, ng, idx.ctypes.data, win.ctypes.data, first.ctypes.data,
                                                   length.ctypes.data, None))
        self._check(self._L.ngsld_decay_map_bins(self._h, nb, dist.ctypes.data, cnt.ctypes.data, mean.ctypes.data, None))
        groups = []
        for g in range(ng):
            bins = self._bin_columns(dist, cnt, mean, names, int(first[g]), int(first[g] + length[g]))
            groups.append({"chr": chr_name[int(idx[g])].decode(), "win_start": int(win[g]), **bins})
        return groups

    def site_ld(self, ld=("r2",), max_kb_dist: float = float("inf"), min_maf: float = 0.0, linked_min: float = 0.5,
                abs_value: bool = True) -> tuple[dict, dict]:
        """Per-site LD summaries of the planned pairs on the device (ngsld_site_ld, SITES.md): (sites, stats).  sites holds
        numpy arrays of n_sites entries: "n" (counted rows) and per statistic F of ld (r2_ExpG, D, Dp, r2) "sum_F" and "max_F"
        (int64 micro-units: value * 10^6), "linked_F" and "mean_F".  Where n is 0, max_F is the smallest int64 and mean_F NaN."""
        return self._site_ld_job(ld, max_kb_dist, min_maf, linked_min, abs_value).run()

    def _site_ld_job(self, ld=("r2",), max_kb_dist: float = float("inf"), min_maf: float = 0.0, linked_min: float = 0.5,
                     abs_value: bool = True) -> _Job:
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        p = SiteLdParams(C.sizeof(SiteLdParams), mask, float(max_kb_dist), float(min_maf), float(linked_min), int(bool(abs_value)), 0)
        st = SiteLdStats()
        st.struct_size = C.sizeof(SiteLdStats)

        def call():
            self._check(self._L.ngsld_site_ld(self._h, C.byref(p), C.byref(st)))

        return _Job(AN_SITE_LD, p, st, call, lambda: self._site_ld_read(st, mask))

    def _site_ld_read(self, st, mask) -> tuple[dict, dict]:
        m = max(self.n_sites, 1)
        sites = {"n": np.zeros(m, dtype=np.uint64)}
        for k, f in enumerate(DECAY_FIELDS):
            if not (mask >> k) & 1:
                continue
            sites[f"sum_{f}"], sites[f"max_{f}"] = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
            sites[f"linked_{f}"], sites[f"mean_{f}"] = np.zeros(m, dtype=np.uint64), np.zeros(m)
            self._check(self._L.ngsld_site_ld_get(self._h, 4 + k, sites["n"].ctypes.data, sites[f"sum_{f}"].ctypes.data,
                                                  sites[f"max_{f}"].ctypes.data, sites[f"linked_{f}"].ctypes.data,
                                                  sites[f"mean_{f}"].ctypes.data))
        sites = {k: v[:self.n_sites] for k, v in sites.items()}
        return sites, {k: getattr(st, k) for k, _ in SiteLdStats._fields_ if k != "struct_size"}

    def scan(self, half_window: int, ld=("r2",), max_kb_dist: float = float("inf"), min_maf: float = 0.0) -> tuple[dict, dict]:
        """The LD scan of the planned pairs on the device (ngsld_scan, SCAN.md): (windows, stats).  windows holds numpy arrays
        of n_sites entries: "win_first" and "win_last" (uint32: the window of a site as a range of site indices), "n_ll", "n_rr",
        "n_lr" (the rows inside the left flank, inside the right flank and across the site) and per statistic F of ld (r2_ExpG,
        D, Dp, r2) "sum_ll_F", "sum_rr_F", "sum_lr_F" (int64 micro-units: |value| * 10^6), "zns_F" and "omega_F" (NaN where
        they are not defined)."""
        return self._scan_job(half_window, ld, max_kb_dist, min_maf).run()

    def _scan_job(self, half_window: int, ld=("r2",), max_kb_dist: float = float("inf"), min_maf: float = 0.0) -> _Job:
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        if not 0 <= int(half_window) < 2 ** 64:
            raise ValueError("half_window must be a non-negative integer")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        p = ScanParams(C.sizeof(ScanParams), mask, int(half_window), float(max_kb_dist), float(min_maf), 0)
        st = ScanStats()
        st.struct_size = C.sizeof(ScanStats)

        def call():
            self._check(self._L.ngsld_scan(self._h, C.byref(p), C.byref(st)))

        return _Job(AN_SCAN, p, st, call, lambda: self._scan_read(st, mask))

    def _scan_read(self, st, mask) -> tuple[dict, dict]:
        m = max(self.n_sites, 1)
        win = {"win_first": np.zeros(m, dtype=np.uint32), "win_last": np.zeros(m, dtype=np.uint32)}
        for cl in ("ll", "rr", "lr"):
            win[f"n_{cl}"] = np.zeros(m, dtype=np.uint64)
        for k, f in enumerate(DECAY_FIELDS):
            if not (mask >> k) & 1:
                continue
            for cl in ("ll", "rr", "lr"):
                win[f"sum_{cl}_{f}"] = np.zeros(m, dtype=np.int64)
            win[f"zns_{f}"], win[f"omega_{f}"] = np.zeros(m), np.zeros(m)
            self._check(self._L.ngsld_scan_get(self._h, 4 + k, win["win_first"].ctypes.data, win["win_last"].ctypes.data,
                                               win["n_ll"].ctypes.data, win["n_rr"].ctypes.data, win["n_lr"].ctypes.data,
                                               win[f"sum_ll_{f}"].ctypes.data, win[f"sum_rr_{f}"].ctypes.data,
                                               win[f"sum_lr_{f}"].ctypes.data, win[f"zns_{f}"].ctypes.data,
                                               win[f"omega_{f}"].ctypes.data))
        win = {k: v[:self.n_sites] for k, v in win.items()}
        return win, {k: getattr(st, k) for k, _ in ScanStats._fields_ if k not in ("struct_size", "reserved")}

    def clusters(self, field: int = 7, min_weight: float = 0.5, max_kb_dist: float = float("inf"), min_maf: float = 0.0,
                 abs_value: bool = True, min_size: int = 2) -> tuple[np.ndarray, dict, dict]:
        """LD clusters of the planned pairs on the device (ngsld_clusters, CLUSTERS.md): (cluster_ids, table, stats).
        cluster_ids holds every site's cluster (uint32; 0: not a node; ids count singletons too).  table holds numpy arrays with
        one entry per cluster of at least min_size sites, in id order: "id", "size", "first", "last", "span", "edges", "sum"
        (int64 micro-units: value * 10^6), "mean" (NaN without edges) and "density" (NaN for a singleton)."""
        return self._clusters_job(field, min_weight, max_kb_dist, min_maf, abs_value, min_size).run()

    def _clusters_job(self, field: int = 7, min_weight: float = 0.5, max_kb_dist: float = float("inf"), min_maf: float = 0.0,
                      abs_value: bool = True, min_size: int = 2) -> _Job:
        p = ClustersParams(C.sizeof(ClustersParams), int(field), float(max_kb_dist), float(min_maf), float(min_weight),
                           int(bool(abs_value)), 0)
        st = ClustersStats()
        st.struct_size = C.sizeof(ClustersStats)

        def call():
            self._check(self._L.ngsld_clusters(self._h, C.byref(p), C.byref(st)))

        return _Job(AN_CLUSTERS, p, st, call, lambda: self._clusters_read(st, min_size))

    def _clusters_read(self, st, min_size) -> tuple[np.ndarray, dict, dict]:
        ids = np.zeros(max(self.n_sites, 1), dtype=np.uint32)
        self._check(self._L.ngsld_clusters_sites(self._h, ids.ctypes.data))
        rows = C.c_uint64(0)
        self._check(self._L.ngsld_clusters_table(self._h, int(min_size), 0, None, None, None, None, None, None, None, None, None,
                                                 C.byref(rows)))
        m = max(int(rows.value), 1)
        kinds = dict(id=np.uint32, size=np.uint32, first=np.uint32, last=np.uint32, span=np.uint64, edges=np.uint64, sum=np.int64,
                     mean=np.float64, density=np.float64)
        table = {k: np.zeros(m, dtype=t) for k, t in kinds.items()}
        self._check(self._L.ngsld_clusters_table(self._h, int(min_size), m, *(table[k].ctypes.data for k in kinds), C.byref(rows)))
        table = {k: v[:int(rows.value)] for k, v in table.items()}
        return ids[:self.n_sites], table, {k: getattr(st, k) for k, _ in ClustersStats._fields_ if k not in ("struct_size", "reserved")}

    def ld_tree(self, field: int = 7, min_weight: float = 0.1, max_kb_dist: float = float("inf"), min_maf: float = 0.0,
                abs_value: bool = True) -> tuple[dict, dict]:
        """The single-linkage LD tree of the planned pairs on the device (ngsld_ld_tree, TREE.md): (merges, stats).  merges holds
        numpy arrays with one entry per merge, in rule order: "s1", "s2" (the edge's sites), "q" (int64 micro-units: value *
        10^6), "dist", "left" and "right" (R's hclust$merge convention: -(site index + 1) for a single site, else the number of
        the merge that made the cluster), "size", "first" and "last".  Engine.ld_tree_cut gives the clusters at any floor >=
        min_weight without another run."""
        p = TreeParams(C.sizeof(TreeParams), int(field), float(max_kb_dist), float(min_maf), float(min_weight), int(bool(abs_value)), 0)
        st = TreeStats()
        st.struct_size = C.sizeof(TreeStats)
        self._check(self._L.ngsld_ld_tree(self._h, C.byref(p), C.byref(st)))
        rows = C.c_uint64(0)
        self._check(self._L.ngsld_ld_tree_merges(self._h, 0, None, None, None, None, None, None, None, None, None, C.byref(rows)))
        m = max(int(rows.value), 1)
        kinds = dict(s1=np.uint32, s2=np.uint32, q=np.int64, dist=np.uint64, left=np.int64, right=np.int64, size=np.uint32,
                     first=np.uint32, last=np.uint32)
        merges = {k: np.zeros(m, dtype=t) for k, t in kinds.items()}
        self._check(self._L.ngsld_ld_tree_merges(self._h, m, *(merges[k].ctypes.data for k in kinds), C.byref(rows)))
        merges = {k: v[:int(rows.value)] for k, v in merges.items()}
        return merges, {k: getattr(st, k) for k, _ in TreeStats._fields_ if k not in ("struct_size", "reserved")}

    def ld_tree_cut(self, t: float) -> np.ndarray:
        """The clusters of the last ld_tree at the floor t >= its min_weight (ngsld_ld_tree_cut): every site's cluster id, what
        Engine.clusters gives at min_weight = t with the other parameters equal.  No device work."""
        ids = np.zeros(max(self.n_sites, 1), dtype=np.uint32)
        self._check(self._L.ngsld_ld_tree_cut(self._h, float(t), ids.ctypes.data, None))
        return ids[:self.n_sites]

    def grid(self, labels: list[str] | None, bin_size: int, ld=("r2",), max_kb_dist: float = float("inf"), min_maf: float = 0.0,
             linked_min: float = 0.5, abs_value: bool = True) -> tuple[dict, dict]:
        """The LD grid of the planned pairs on the device (ngsld_grid, GRID.md): (cells, stats).  cells holds numpy arrays with
        one entry per cell with rows, ordered by chromosome (file order), bin1, bin2: "chr" (the chromosome's name), "bin1" and
        "bin2" (the lower breaks b * bin_size of the windows of the pair's first and second site, as --grid_out writes them), "n"
        (counted rows) and per statistic F of ld (r2_ExpG, D, Dp, r2) "sum_F" and "max_F" (int64 micro-units: value * 10^6),
        "linked_F" and "mean_F"."""
        return self._grid_job(labels, bin_size, ld, max_kb_dist, min_maf, linked_min, abs_value).run()

    def _grid_job(self, labels: list[str] | None, bin_size: int, ld=("r2",), max_kb_dist: float = float("inf"),
                  min_maf: float = 0.0, linked_min: float = 0.5, abs_value: bool = True) -> _Job:
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        arr = None if labels is None else (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels])
        p = GridParams(C.sizeof(GridParams), mask, int(bin_size), float(max_kb_dist), float(min_maf), float(linked_min),
                       int(bool(abs_value)), 0)
        st = GridStats()
        st.struct_size = C.sizeof(GridStats)

        def call():
            self._check(self._L.ngsld_grid(self._h, C.byref(p), arr, C.byref(st)))

        return _Job(AN_GRID, p, st, call, lambda: self._grid_read(st, mask, bin_size), labels=arr)

    def _grid_read(self, st, mask, bin_size) -> tuple[dict, dict]:
        nc = int(st.cells)
        m = max(nc, 1)
        n_chr = C.c_uint64(0)
        self._check(self._L.ngsld_grid_chromosomes(self._h, 0, None, C.byref(n_chr)))
        names = (C.c_char_p * max(int(n_chr.value), 1))()
        self._check(self._L.ngsld_grid_chromosomes(self._h, int(n_chr.value), names, None))
        names = np.array([names[k].decode() for k in range(int(n_chr.value))] or [""])
        idx, b1, b2 = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        cells = {"n": np.zeros(m, dtype=np.uint64)}
        got = C.c_uint64(0)
        self._check(self._L.ngsld_grid_cells(self._h, m, idx.ctypes.data, b1.ctypes.data, b2.ctypes.data, cells["n"].ctypes.data,
                                             C.byref(got)))
        assert got.value == nc
        cells = {"chr": names[idx], "bin1": b1 * np.uint64(int(bin_size)), "bin2": b2 * np.uint64(int(bin_size)), **cells}
        for k, f in enumerate(DECAY_FIELDS):
            if not (mask >> k) & 1:
                continue
            cells[f"sum_{f}"], cells[f"max_{f}"] = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
            cells[f"linked_{f}"], cells[f"mean_{f}"] = np.zeros(m, dtype=np.uint64), np.zeros(m)
            self._check(self._L.ngsld_grid_get(self._h, 4 + k, m, cells[f"sum_{f}"].ctypes.data, cells[f"max_{f}"].ctypes.data,
                                               cells[f"linked_{f}"].ctypes.data, cells[f"mean_{f}"].ctypes.data))
        cells = {k: v[:nc] for k, v in cells.items()}
        return cells, {k: getattr(st, k) for k, _ in GridStats._fields_ if k != "struct_size"}

    def cross_ld(self, labels: list[str] | None, bin_size: int = 0, ld=("r2",), min_maf: float = 0.0, linked_min: float = 0.5,
                 abs_value: bool = True, within: bool = True, min_kb_dist: float = 0.0) -> tuple[dict, dict]:
        """LD across chromosomes of the planned pairs on the device (ngsld_cross_ld, CROSS.md): (cells, stats).  cells holds
        numpy arrays with one entry per cell with rows, ordered by the bin of the pair's first site, then of its second, the bins
        numbered consecutively over the chromosomes: "chr1" and "chr2" (the chromosomes' names; with bin_size 0 labels may be
        None, the names are then "1", "2", ...), "bin1" and "bin2" (the lower breaks b * bin_size of the two windows; 0 with
        bin_size 0: one bin per chromosome), "n" (counted rows) and per statistic F of ld what Engine.grid gives per cell."""
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        arr = None if labels is None else (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels])
        p = CrossLdParams(C.sizeof(CrossLdParams), mask, int(bin_size), float(min_maf), float(linked_min), float(min_kb_dist),
                          int(bool(abs_value)), int(bool(within)))
        st = CrossLdStats()
        st.struct_size = C.sizeof(CrossLdStats)
        self._check(self._L.ngsld_cross_ld(self._h, C.byref(p), arr, C.byref(st)))
        nc = int(st.cells)
        m = max(nc, 1)
        n_chr = C.c_uint64(0)
        self._check(self._L.ngsld_cross_ld_chromosomes(self._h, 0, None, C.byref(n_chr)))
        names = (C.c_char_p * max(int(n_chr.value), 1))()
        self._check(self._L.ngsld_cross_ld_chromosomes(self._h, int(n_chr.value), names, None))
        names = np.array([names[k].decode() for k in range(int(n_chr.value))] or [""])
        i1, i2 = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
        b1, b2 = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        cells = {"n": np.zeros(m, dtype=np.uint64)}
        got = C.c_uint64(0)
        self._check(self._L.ngsld_cross_ld_cells(self._h, m, i1.ctypes.data, b1.ctypes.data, i2.ctypes.data, b2.ctypes.data,
                                                 cells["n"].ctypes.data, C.byref(got)))
        assert got.value == nc
        B = np.uint64(int(bin_size))
        cells = {"chr1": names[i1], "bin1": b1 * B, "chr2": names[i2], "bin2": b2 * B, **cells}
        for k, f in enumerate(DECAY_FIELDS):
            if not (mask >> k) & 1:
                continue
            cells[f"sum_{f}"], cells[f"max_{f}"] = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
            cells[f"linked_{f}"], cells[f"mean_{f}"] = np.zeros(m, dtype=np.uint64), np.zeros(m)
            self._check(self._L.ngsld_cross_ld_get(self._h, 4 + k, m, cells[f"sum_{f}"].ctypes.data, cells[f"max_{f}"].ctypes.data,
                                                   cells[f"linked_{f}"].ctypes.data, cells[f"mean_{f}"].ctypes.data))
        cells = {k: v[:nc] for k, v in cells.items()}
        return cells, {k: getattr(st, k) for k, _ in CrossLdStats._fields_ if k != "struct_size"}

    def analyze(self, prune: dict | None = None, decay: dict | None = None, site_ld: dict | None = None,
                clusters: dict | None = None, grid: dict | None = None, scan: dict | None = None) -> tuple[dict, dict]:
        """Several analyses over one run of the pair kernels (ngsld_analyze, ANALYZE.md): (results, stats).  Each argument is a
        dict of the keyword arguments of the method of that name (None: not asked for); results[name] is exactly what that
        method returns.  The list goes to the library in the order of this signature."""
        asked = [("prune", prune), ("decay", decay), ("site_ld", site_ld), ("clusters", clusters), ("grid", grid), ("scan", scan)]
        jobs = {name: getattr(self, f"_{name}_job")(**kw) for name, kw in asked if kw is not None}
        arr = (Analysis * max(len(jobs), 1))()
        for a, job in zip(arr, jobs.values()):
            a.struct_size, a.kind = C.sizeof(Analysis), job.kind
            a.params, a.stats = C.addressof(job.params), C.addressof(job.stats)
            if job.labels is not None:
                a.labels = C.cast(job.labels, C.POINTER(C.c_char_p))
            if job.site_state is not None:
                a.site_state = job.site_state.ctypes.data
        st = AnalyzeStats()
        st.struct_size = C.sizeof(AnalyzeStats)
        self.analyze_stats = st  # (what a refused call reports: pairs_run stays 0 when the pair kernels never started)
        self._check(self._L.ngsld_analyze(self._h, arr, len(jobs), C.byref(st)))
        results = {name: job.read() for name, job in jobs.items()}
        return results, {k: getattr(st, k) for k, _ in AnalyzeStats._fields_ if k != "struct_size"}

    def linked_pairs(self, labels: list[str] | None = None, field: int = 7, min_weight: float = 0.5, abs_value: bool = True,
                     max_kb_dist: float = float("inf"), min_maf: float = 0.0, records: bool = True, text: bool = False,
                     on_batch=None) -> tuple[dict, dict]:
        """The linked pairs of the planned table on the device (ngsld_linked_pairs, LINKED.md): (result, stats).  result holds
        the rows of the TSV that pass the filter, in the table's order, the batches concatenated: with records "s1" and "s2"
        (uint32), "std" (REC_STD) and, iff the plan has extend_out, "ext" (REC_EXT); with text "text" (bytes: each row as the
        full table prints it; labels None = "(null)").  on_batch (optional): called with the number of batches so far after
        each one; a non-zero return ends the call, which then raises NgsldError with that code."""
        arr = None if labels is None else (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels])
        want = (LINKED_RECORDS if records else 0) | (LINKED_TEXT if text else 0)
        p = LinkedParams(C.sizeof(LinkedParams), int(field), float(min_weight), float(max_kb_dist), float(min_maf),
                         int(bool(abs_value)), want)
        st = LinkedStats()
        st.struct_size = C.sizeof(LinkedStats)
        got = dict(s1=[], s2=[], std=[], ext=[], text=[])
        calls = [0]

        def sink(_user, bp):
            b = bp.contents
            k = int(b.n)
            if b.s1:
                got["s1"].append(np.frombuffer(C.string_at(b.s1, k * 4), dtype=np.uint32).copy())
                got["s2"].append(np.frombuffer(C.string_at(b.s2, k * 4), dtype=np.uint32).copy())
                got["std"].append(np.frombuffer(C.string_at(b.std, k * REC_STD.itemsize), dtype=REC_STD).copy())
                if b.ext:
                    got["ext"].append(np.frombuffer(C.string_at(b.ext, k * REC_EXT.itemsize), dtype=REC_EXT).copy())
            if b.text:
                got["text"].append(C.string_at(b.text, b.text_len))
            calls[0] += 1
            return int(on_batch(calls[0])) if on_batch is not None else 0

        self._check(self._L.ngsld_linked_pairs(self._h, C.byref(p), arr, LINKED_FN(sink), None, C.byref(st)))
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)  # noqa: E731
        result = {}
        if records:
            result.update(s1=cat(got["s1"], np.uint32), s2=cat(got["s2"], np.uint32), std=cat(got["std"], REC_STD))
            if self.extend_out:
                result["ext"] = cat(got["ext"], REC_EXT)
        if text:
            result["text"] = b"".join(got["text"])
        stats = {k: getattr(st, k) for k, _ in LinkedStats._fields_ if k not in ("struct_size", "reserved")}
        stats["batches"] = calls[0]
        return result, stats

    def partners(self, k: int, field: int = 7, min_weight: float = 0.5, abs_value: bool = True, max_kb_dist: float = float("inf"),
                 min_maf: float = 0.0, query=None) -> tuple[dict, dict]:
        """Every site's top-k LD partners of the planned table on the device (ngsld_partners, PARTNERS.md): (result, stats).
        result holds "rows" (uint64[n]: the site's partner rows before the cut to k), "partner" (int64[n, k]: site indices in
        rank order, -1 for none), "value_micro" (int64[n, k]: the printed value * 10^6, |value| with abs_value) and "value"
        (float64[n, k]: value_micro / 1e6, NaN for none).  query (optional): one entry per site, a site collects partners iff
        its entry is not 0; any site can be a partner."""
        p = PartnersParams(C.sizeof(PartnersParams), int(k), int(field), int(bool(abs_value)), float(min_weight),
                           float(max_kb_dist), float(min_maf))
        st = PartnersStats()
        st.struct_size = C.sizeof(PartnersStats)
        q = None
        if query is not None:
            q = np.ascontiguousarray(np.asarray(query) != 0, dtype=np.uint8)
            if q.shape != (self.n_sites,):
                raise ValueError(f"query must have one entry per site ({self.n_sites}): {q.shape}")
        self._check(self._L.ngsld_partners(self._h, C.byref(p), None if q is None else q.ctypes.data, C.byref(st)))
        kk, n, f = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self._check(self._L.ngsld_partners_info(self._h, C.byref(kk), C.byref(n), C.byref(f)))
        n, kk = int(n.value), int(kk.value)
        rows = np.zeros(n, dtype=np.uint64)
        partner = np.zeros((n, kk), dtype=np.uint32)
        value_micro = np.zeros((n, kk), dtype=np.int64)
        self._check(self._L.ngsld_partners_get(self._h, rows.ctypes.data, partner.ctypes.data, value_micro.ctypes.data))
        none = partner == 0xFFFFFFFF
        result = dict(rows=rows, partner=np.where(none, -1, partner.astype(np.int64)), value_micro=value_micro,
                      value=np.where(none, np.nan, value_micro / 1e6))
        return result, {k_: getattr(st, k_) for k_, _ in PartnersStats._fields_ if k_ not in ("struct_size", "reserved")}

    def blocks(self, labels: list[str], chr: str, start: int, end: int,
               ld=("r2", "Dp")) -> tuple[np.ndarray, dict, dict]:
        """LD block matrices of one region on the device (ngsld_blocks, BLOCKS.md): (sites, {stat: (values, present)}, stats).
        sites are the matrix sites' indices in matrix order; values[a, b] is the record's double of the pair (a, b) (NaN where
        present[a, b] is 0); stats are r2_ExpG, D, Dp, r2.  blocks_text(stat) then gives the matrix as a file."""
        ld = (ld,) if isinstance(ld, str) else tuple(ld)
        bad = [f for f in ld if f not in DECAY_FIELDS]
        if bad or not ld:
            raise ValueError(f"ld must name some of {DECAY_FIELDS}: {bad}")
        mask = sum(1 << DECAY_FIELDS.index(f) for f in set(ld))
        arr = (C.c_char_p * max(len(labels), 1))(*[l.encode() for l in labels]) if labels is not None else None
        p = BlocksParams(C.sizeof(BlocksParams), mask, chr.encode(), int(start), int(end))
        st = BlocksStats()
        st.struct_size = C.sizeof(BlocksStats)
        self._check(self._L.ngsld_blocks(self._h, C.byref(p), arr, C.byref(st)))
        m = st.sites
        sites = np.zeros(max(m, 1), dtype=np.uint64)
        got = C.c_uint64()
        self._check(self._L.ngsld_blocks_sites(self._h, m, sites.ctypes.data, C.byref(got)))
        assert got.value == m
        mats = {}
        for k, f in enumerate(DECAY_FIELDS):
            if not (mask >> k) & 1:
                continue
            values = np.zeros((m, m))
            present = np.zeros((m, m), dtype=np.uint8)
            if m:
                self._check(self._L.ngsld_blocks_matrix(self._h, 4 + k, values.ctypes.data, present.ctypes.data))
            mats[f] = (values, present)
        return sites[:m].astype(np.int64), mats, {k: getattr(st, k) for k, _ in BlocksStats._fields_
                                                  if k not in ("struct_size", "reserved")}

    def blocks_text(self, field: str, stats: dict | None = None) -> bytes:
        """One statistic's matrix of the last blocks() as a file (ngsld_blocks_text).  stats (optional dict): gets the call's
        format_ms, host_rows and the number of pieces the sink received ("pieces")."""
        parts = []

        def sink(_user, text, n):
            parts.append(C.string_at(text, n))
            return 0

        st = BlocksStats()
        st.struct_size = C.sizeof(BlocksStats)
        self._check(self._L.ngsld_blocks_text(self._h, 4 + DECAY_FIELDS.index(field), TEXT_FN(sink), None, C.byref(st)))
        if stats is not None:
            stats.update(format_ms=st.format_ms, host_rows=st.host_rows, pieces=len(parts))
        return b"".join(parts)
