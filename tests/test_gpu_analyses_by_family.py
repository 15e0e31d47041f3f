"""The seven record passes -- LD pruning, decay, blocks, site LD, clusters, the LD grid and the linked pairs -- under every
pair-kernel family.

The seven analyses' own files hold each pass, bit for bit, to its plain-Python rule (prune_ref, decay_ref, blocks_ref, site_ref,
cluster_ref, grid_ref, linked_ref) applied to the engine's own TSV, on cohorts of 4 to 500 individuals: the 8-lane group kernel, the run kernel at 8
slots, the called-genotype kernel -- all run families, whose items span 64 candidates.  Here the same checks, with the same
comparison functions, run where the pairs come from the other families: 16- and 32-lane groups, the run kernel's last P-form shape, the
a/b run kernel, the multi-wavefront kernel in both forms (with --ignore_miss_data too, and with un-called monomorphic sites) and both streaming kernels.  The last
four are launched item by item, not through the run list, and their items are 4 x pairs_per_item or pairs_per_item
candidates wide: with pairs_per_item 5 no row is a whole number of items and every item is shorter than a wavefront.

What the restatements cannot see -- they read the engine's TSV, so an item dropped by the pair launch is gone from both sides --
is checked apart from the engine: the TSV's (site1, site2, dist) columns against a plain enumeration of the window, and some
20 rows per multi-wavefront and streaming case against the oracle's own records of the two sites.

LD pruning's chunk loop is under test too: NGSLD_TEST_PRUNE_CHUNK_PAIRS cuts its record pass (RecordPass, the one the other
passes go through) at a tenth of the pairs in the chunk cuts below, where site_state keeps its bytes and is held to prune_ref
again; its stats carry no chunk count, so that it ran in chunks is shown in tests/test_gpu_record_pass_large.py, from the pairs
of the last ngsld_run_device, with the edge arrays regrown from chunk to chunk and the refusal of a row beyond the chunk.

The linked pairs are compared with more than the TSV: their 32 B and 40 B records must be the bytes of Engine.run's records of
those pairs (test_gpu_linked.Table, built once per engine).  Where items are 5 or 20 candidates wide a row of the table spans
many items, and the cuts assert from the plan's items that the linked rows do lie where the survivor placement can go wrong: in
items shorter than the span, in three and more items of one row, in an item's last candidate, in masks with a hole -- and that
a cell of the grid takes rows from two items of one row.

GPU time of this file on one MI355X: see README.md (the tests row)."""
import functools
import math
import os

import numpy as np
import pytest

import cluster_ref
import decay_ref
import printed_values
import prune_ref
import site_ref
from ngsld_amd import capi, shard, synth
from oracle import orc
from test_gpu_blocks import Run as _BlocksRun, check as _blocks_check
from test_gpu_clusters import _floor, _same as _same_clusters
from test_gpu_decay import _same as _same_decay
from test_gpu_grid import _check as _grid_check  # (that file imports this one inside a test only: no cycle at collection)
from test_gpu_linked import Table as _LinkedTable, _check as _linked_check, _chunks as _linked_chunks
from test_gpu_site_ld import _same as _same_site_ld

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
WIN = dict(max_kb_dist=20, extend_out=True)
LIMIT = 20_000
PRUNE_KW = dict(min_weight=0.3, weight_type="a")  # (test_gpu_prune.py's floor from 500 individuals on)
DECAY_KW = dict(ld=ALL4, bin_size=33.3)
SITE_KW = dict(ld=ALL4, abs_value=False, linked_min=0.3)
GRID_BIN = 2000
GRID_KW = dict(ld=ALL4, abs_value=False, linked_min=0.3)
# the linked pairs' two settings: absolute r2; signed D with a limit inside the window and the maf filter.  The floors are set by
# what these inputs hold (the oracle's tables of the called inputs, looked at on the CPU).  r2 falls smoothly with the candidate:
# 0.9 at a site's neighbour, 0.3 at the 12th, 0.03 at the 40th, noise of some 0.002 from the 60th on -- at a floor of 0.3 every
# linked row of a site lies in its first item, even of 20 candidates, and the masks are prefixes.  At 0.005 the floor is crossed
# between the 45th and the 60th candidate, where the noise leaves the masks ragged, and rows beyond survive here and there.  Within
# 7.5 kb D is below -0.02 in no pair of 1,000 individuals or more and the smallest maf of n1000, n1500 and n5121 is 0.22, so
# floors of -0.02 and 0.1 filter nothing there: 0.02 is crossed around the 40th candidate (and drops the negative values that n100
# and n700 do hold inside the limit), and 0.27 drops between a fiftieth and a seventh of the sites -- whole rows, and single
# candidates out of every item they lie in.
LINKED_KW = {
    "abs_r2": dict(field=7, min_weight=0.005),
    "signed_D": dict(field=5, abs_value=False, min_weight=0.02, max_kb_dist=7.5, min_maf=0.27),
}
CHUNK_KNOBS = ("NGSLD_TEST_DECAY_CHUNK_PAIRS", "NGSLD_TEST_SITE_CHUNK_PAIRS", "NGSLD_TEST_CLUSTER_CHUNK_PAIRS",
               "NGSLD_TEST_PRUNE_CHUNK_PAIRS", "NGSLD_TEST_GRID_CHUNK_PAIRS", "NGSLD_TEST_LINKED_CHUNK_PAIRS")
KNOBS = CHUNK_KNOBS + ("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", "NGSLD_TEST_SITE_LDS_BYTES", "NGSLD_TEST_DECAY_LDS_BYTES",
                       "NGSLD_TEST_BLOCKS_HOST_ROWS", "NGSLD_TEST_BLOCKS_TEXT_ROWS", "NGSLD_TEST_GRID_LDS_BYTES",
                       "NGSLD_TEST_LINKED_FORCE_HOST", "NGSLD_TEST_RECORD_SLICE_ITEMS")
SPOT_PAIRS, SPOT_SEED = 20, 5

# input: (n_sites, n_ind, synth kw, individuals without data).  Depth 4 as in the five files, but for the un-called monomorphic
# sites: at 4 reads a site, 1,000 individuals always hold error reads, no estimated frequency reaches 0 and the table has no
# non-finite row (the oracle's has none either); at 60 reads the likelihoods of a monomorphic site are decisive, and the oracle's
# table of these two inputs holds some 12,000 rows with inf and 460 / 697 with nan (test_gpu_replay_lkl.py raises the depth of
# large cohorts for the same reason)
INPUTS = {
    "n100": (400, 100, {}, False),
    "n160": (400, 160, {}, False),
    "n640": (400, 640, {}, False),
    "n700": (400, 700, {}, False),
    "n1000": (400, 1000, {}, False),
    "n1000_mono": (400, 1000, dict(mono_frac=0.2, depth=60.0), False),
    "n1500": (400, 1500, {}, False),
    "n1500_mono": (400, 1500, dict(mono_frac=0.2, depth=60.0), False),
    "n1500_masked": (400, 1500, {}, True),
    "n5121": (300, 5121, {}, False),
}
# case: (input, NGSLD_PAIR_KERNEL, pair_kernel(), describe_dispatch of the cohort, item span at 16 pairs per item)
CASES = {
    "group16": ("n100", None, "group", "group 1x7 lanes=16 np=112", 64),
    "group32": ("n160", None, "group", "group 1x5 lanes=32 np=160", 64),
    "run10": ("n640", None, "run", "run 1x10 lanes=64 np=640", 64),
    "ab": ("n700", None, "ab", "ab 1x11 lanes=64 np=704", 64),
    "multi": ("n1000", None, "multi", "multi 2x8 lanes=64 np=1024", 64),
    "multi_mono": ("n1000_mono", None, "multi", "multi 2x8 lanes=64 np=1024", 64),
    "multi-ab": ("n1500", None, "multi-ab", "multi-ab 2x12 lanes=64 np=1536", 64),
    "multi-ab_mono": ("n1500_mono", None, "multi-ab", "multi-ab 2x12 lanes=64 np=1536", 64),
    "multi-ab_masked": ("n1500_masked", None, "multi-ab", "multi-ab 2x12 lanes=64 np=1536", 64),
    # (left alone, 5,121 individuals take eight wavefronts per pair in the a/b form: the streaming kernels are asked for)
    "stream_resident": ("n5121", "bres", "stream", "multi-ab 8x11 lanes=64 np=5632", 16),
    "stream_plain": ("n5121", "stream", "stream", "multi-ab 8x11 lanes=64 np=5632", 16),
}
SPOT_CASES = ["multi", "multi-ab", "stream_resident", "stream_plain"]


class Input:
    def __init__(self, name):
        n_sites, self.n_ind, skw, self.masked = INPUTS[name]
        self.raw = synth.make_gl_numpy(n_sites, self.n_ind, 900 + n_sites + self.n_ind, **{"depth": 4.0, **skw})
        if self.masked:  # (three equal likelihoods: an individual without data at any site)
            self.raw[:, np.random.default_rng(1500).random(self.n_ind) < 0.1] = 1.0 / 3.0
        self.chrs, self.pos = synth.make_positions(n_sites, 41, max_gap=300, n_chr=2)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(self.chrs, self.pos)]
        # every pair of the window, row by row: the rule of plan_rows and of the reference's loop (ngsLD.cpp:252) -- same
        # chromosome, dist <= the limit (not strict); tests/test_stream_host.py holds ngsld_window_ends to that loop's walk
        self.keys = [(i, j) for i in range(n_sites) for j in range(i + 1, n_sites)
                     if self.chrs[i] == self.chrs[j] and self.pos[j] - self.pos[i] <= LIMIT]
        # a region strictly inside chr1 that starts and ends mid-row-range: rows are left out on both sides
        p1 = np.sort(np.array([p for c, p in zip(self.chrs, self.pos) if c == "chr1"]))
        self.region = (int(p1[len(p1) // 4]) + 1, int(p1[len(p1) * 3 // 5]))
        member = [c == "chr1" and self.region[0] <= p <= self.region[1] for c, p in zip(self.chrs, self.pos)]
        self.member_pairs = sum(1 for i, _ in self.keys if member[i])

    def key_columns(self):
        return [(self.labels[i], self.labels[j], str(int(self.pos[j] - self.pos[i]))) for i, j in self.keys]


@functools.lru_cache(maxsize=4)
def _input(name):
    return Input(name)


def _new_engine(inp, how):
    """A context on the input; how: NGSLD_PAIR_KERNEL around its creation (read there and nowhere else), put back after."""
    before = os.environ.get("NGSLD_PAIR_KERNEL")
    try:
        if how is not None:
            os.environ["NGSLD_PAIR_KERNEL"] = how
        eng = capi.Engine(0)
    finally:
        os.environ.pop("NGSLD_PAIR_KERNEL", None)
        if before is not None:
            os.environ["NGSLD_PAIR_KERNEL"] = before
    eng.set_geno_raw(inp.raw, ignore_miss_data=inp.masked)
    eng.set_pos_dist(shard.pos_dist_from_positions(inp.chrs, inp.pos))
    return eng


def _plan(eng, inp):
    return eng.plan(ignore_miss_data=inp.masked, **WIN)


def _items(eng):
    """(s1, count) of every work item of the plan."""
    items = eng.items()
    return items["s1"], items["count"]


def _tsv(eng, inp):
    eng.set_text_output(inp.labels)
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _rows(text):
    return [ln for ln in text.splitlines() if ln and not ln.startswith("site1\t")]


# ---- the restatements, once per TSV ----
@functools.lru_cache(maxsize=None)
def _want(text, labels, what, floor=None):
    labels = list(labels)
    if what == "prune":
        return prune_ref.prune_tsv(text, **PRUNE_KW)
    if what == "decay":
        return decay_ref.decay_bins(text, **DECAY_KW)
    if what == "site_ld":
        return site_ref.site_ld(text, labels, **SITE_KW)
    if what == "floor":
        return _floor(text, labels, {})
    assert what == "clusters"
    return cluster_ref.clusters(text, labels, min_size=1, min_weight=floor)


class _Table(_LinkedTable):
    """test_gpu_linked.Table with the rule applied once per setting: the cuts ask for the same rows many times."""

    def want(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self.__dict__.setdefault("_wanted", {}):
            self._wanted[key] = super().want(**kw)
        return self._wanted[key]


class Sub:
    """An engine with its plan, its input and its own TSV: what an analysis is run on and checked against."""

    mono = False

    def __init__(self, eng, inp, text):
        self.eng, self.inp, self.text = eng, inp, text
        self.labels = tuple(inp.labels)
        self.n_pairs = len(inp.keys)
        self._table = None
        self.items = None  # (Engine.items() of the plan, where a check needs them: the cuts set them)

    @property
    def floor(self):
        return _want(self.text, self.labels, "floor")

    @property
    def table(self):
        """The records of Engine.run and the rows of run_text (test_gpu_linked.Table): one extra run of each per engine, made at
        the first use and left unchanged.  Its rows are the TSV's; the engine is left writing text, as _tsv left it."""
        if self._table is None:
            self._table = _Table(self.eng, self.inp.labels)
            self.eng.set_text_output(self.inp.labels)
            assert self._table.text == self.text and self._table.ext is not None
            assert [(int(a), int(b)) for a, b in zip(self._table.s1, self._table.s2)] == self.inp.keys
        return self._table

    @functools.cached_property
    def columns(self):
        """The TSV's r2_ExpG, D, Dp, r2 and maf1, maf2 as float() reads them: one row of six per row of the table."""
        got = np.array([[float(f[k]) for k in (3, 4, 5, 6, 8, 9)] for f in (ln.split("\t") for ln in _rows(self.text))])
        assert got.shape == (self.n_pairs, 6)
        return got

    @property
    def grid_counted(self):
        """The rows GRID_KW counts (grid_ref: dist finite -- every planned pair's is --, both maf and all four statistics finite)."""
        return np.isfinite(self.columns).all(axis=1)


def _run_prune(s):
    return s.eng.prune(s.inp.labels, **PRUNE_KW)


def _check_prune(s, res):
    state, stats = res
    kept, excl = _want(s.text, s.labels, "prune")
    got_kept = {s.inp.labels[k] for k in np.nonzero(state == 1)[0]}
    got_excl = {s.inp.labels[k] for k in np.nonzero(state == 2)[0]}
    assert got_kept == kept and got_excl == excl, (len(got_kept ^ kept), len(got_excl ^ excl))
    assert stats["nodes"] == stats["kept"] + stats["excluded"] == len(kept) + len(excl)
    assert stats["pairs"] == s.n_pairs and stats["edges"] > 0 and stats["excluded"] > 0
    return f"prune: pairs {stats['pairs']} nodes {stats['nodes']} edges {stats['edges']} excluded {stats['excluded']}"


def _run_decay(s):
    return s.eng.decay(**DECAY_KW)


def _check_decay(s, res):
    bins, stats = res
    want = _want(s.text, s.labels, "decay")
    _same_decay(bins, want, ALL4)
    assert stats["bins"] == len(want) > 0 and stats["pairs_counted"] == sum(w[1] for w in want) > 0
    assert stats["pairs"] == s.n_pairs
    return f"decay: pairs {stats['pairs']} counted {stats['pairs_counted']} bins {stats['bins']} lds {stats['lds']} chunks {stats['chunks']}"


def _run_blocks(s):
    class R:
        pass
    r = R()
    r.eng, r.labels, r.tsv, r.chrs, r.pos = s.eng, s.inp.labels, s.text, s.inp.chrs, s.inp.pos
    r.row_off, _ = s.eng.plan_rows()
    r.member_pairs = lambda c, a, b: _BlocksRun.member_pairs(r, c, a, b)
    # (check: Engine.blocks against blocks_ref on the TSV -- the files byte for byte, the sites, the counts)
    st = _blocks_check(r, "chr1", s.inp.region[0], s.inp.region[1], ALL4)
    sites, mats, _ = s.eng.blocks(s.inp.labels, "chr1", s.inp.region[0], s.inp.region[1], ld=ALL4)
    return sites, mats, {f: s.eng.blocks_text(f) for f in ALL4}, st


def _check_blocks(s, res):
    sites, _, _, st = res  # (held to the restatement where it was run)
    assert st["pairs"] == s.inp.member_pairs and 0 < st["pairs_in_region"] < st["pairs"] < s.n_pairs and st["sites"] == len(sites) > 20
    return f"blocks: sites {st['sites']} pairs {st['pairs_in_region']} of {st['pairs']} chunks {st['chunks']}"


def _run_site_ld(s):
    return s.eng.site_ld(**SITE_KW)


def _check_site_ld(s, res):
    sites, stats = res
    want = _want(s.text, s.labels, "site_ld")
    _same_site_ld(sites, want, ALL4)
    assert stats["pairs"] == s.n_pairs
    assert stats["pairs_counted"] * 2 == sum(want["n"]) > 0 and stats["sites_with_pairs"] == sum(1 for x in want["n"] if x)
    return f"site_ld: pairs {stats['pairs']} counted {stats['pairs_counted']} lds {stats['lds']} chunks {stats['chunks']}"


def _run_clusters(s):
    return s.eng.clusters(min_size=1, min_weight=s.floor)


def _check_clusters(s, res):
    ids, table, stats = res
    want_ids, want_all = _want(s.text, s.labels, "clusters", s.floor)
    _same_clusters(ids, table, want_ids, want_all)
    assert stats["pairs"] == s.n_pairs
    assert stats["nodes"] == sum(1 for k in want_ids if k) and stats["edges"] == sum(r["edges"] for r in want_all)
    assert stats["clusters"] == len(want_all) == max(want_ids, default=0)
    assert stats["clusters_multi"] == sum(1 for r in want_all if r["size"] >= 2)
    assert stats["largest"] == max((r["size"] for r in want_all), default=0)
    slice_items = os.environ.get("NGSLD_TEST_RECORD_SLICE_ITEMS")
    if slice_items is None:
        assert stats["union_launches"] == stats["chunks"]
    else:
        # a launch per slice of a chunk's items (ngsld.h: one per chunk, per 2^24 work items of it; the knob puts fewer in a slice):
        # RecordPass's chunks restated from plan_rows(), as tests/test_gpu_record_pass_large.py holds the pass to them
        row_off = [int(x) for x in s.eng.plan_rows()[0]]
        item_off = np.searchsorted(s.items["s1"], np.arange(len(row_off)))
        chunks = _linked_chunks(row_off, int(os.environ.get("NGSLD_TEST_CLUSTER_CHUNK_PAIRS", row_off[-1])))
        assert len(chunks) == stats["chunks"]
        assert stats["union_launches"] == sum(-(-int(item_off[r1] - item_off[r0]) // int(slice_items)) for r0, r1, _ in chunks) > stats["chunks"]
    return (f"clusters: floor {s.floor} pairs {stats['pairs']} nodes {stats['nodes']} edges {stats['edges']} clusters {stats['clusters']} "
            f"largest {stats['largest']} chunks {stats['chunks']}")


def _run_grid(s):
    # (check: Engine.grid against grid_ref on the TSV -- every cell's key, n, sum, max and linked as integers, the means bit for bit)
    cells, stats, _ = _grid_check(s.eng, s.text, s.inp.labels, GRID_BIN, **GRID_KW)
    return cells, stats


def _check_grid(s, res):
    cells, stats = res  # (held to the restatement where it was run)
    assert stats["pairs"] == s.n_pairs and stats["pairs_counted"] == int(s.grid_counted.sum()) > 0
    assert stats["cells"] == len(cells["n"]) > 0 and int(cells["n"].sum()) == stats["pairs_counted"]
    if "NGSLD_TEST_GRID_LDS_BYTES" not in os.environ:
        assert stats["lds"] == 1
    return (f"grid: pairs {stats['pairs']} counted {stats['pairs_counted']} cells {stats['cells']} band {stats['band']} lds {stats['lds']} "
            f"chunks {stats['chunks']}")


def _run_linked(s):
    """Both settings through test_gpu_linked._check: records + text, records only, text only -- the text the rule's rows as bytes,
    s1, s2, std and ext the bytes of Engine.run's records of those pairs.  On un-called input also every column with non-finite
    rows at a floor of -inf: every finite row and no other, so that every replayed pair with a finite value is among the rows whose
    records are compared."""
    tab = s.table
    res, stats, mono = {}, {}, {}
    for name, kw in LINKED_KW.items():
        res[name], stats[name] = _linked_check(s.eng, tab, **kw)
    if s.mono:
        for f in (4, 5, 6, 7):
            finite = np.isfinite(s.columns[:, f - 4])
            if finite.all():
                continue
            res_f, st_f = _linked_check(s.eng, tab, field=f, min_weight=-math.inf, abs_value=False)
            assert res_f["text"] == "".join(tab.rows[k] + "\n" for k in np.flatnonzero(finite)).encode()
            mono[f] = (st_f["rows"], int((~finite).sum()))
            stats[f"column {f} at -inf"] = st_f
    first = stats["abs_r2"]
    return res, mono, {"chunks": first["chunks"], "pairs": first["pairs"], "settings": stats}


def _check_linked(s, res):
    got, mono, stats = res
    per = stats["settings"]
    assert all(st["pairs"] == s.n_pairs and st["chunks"] == stats["chunks"] for st in per.values())
    host = os.environ.get("NGSLD_TEST_LINKED_FORCE_HOST") == "1"
    for name in LINKED_KW:
        st, ext = per[name], got[name]["ext"]
        assert 0 < st["rows"] < st["pairs"], (name, st["rows"])
        assert st["host_rows"] == (st["rows"] if host else 0), (name, st["host_rows"])
        if s.mono:  # (the 40 B records of the linked rows are not one constant: n_iter is the pair's own)
            assert len(np.unique(ext["n_iter"])) > 1, name
        if s.inp.masked:  # (the individuals without data are in no pair's count)
            assert (ext["n_ind_data"] < s.inp.n_ind).all() and (ext["n_ind_data"] > 0).all(), name
    if s.mono:
        assert mono and all(0 < rows == s.n_pairs - bad for rows, bad in mono.values()), mono
    return ("linked: pairs " + str(stats["pairs"]) + "".join(f", {name} rows {per[name]['rows']} bytes {per[name]['text_bytes']}" for name in LINKED_KW)
            + f" host_rows {sum(per[name]['host_rows'] for name in LINKED_KW)}"
            + (f", finite rows / non-finite at -inf by column {mono}" if s.mono else "") + f" chunks {stats['chunks']}")


def _linked_bytes(res):
    return {f"{name}_{k}": (v if k == "text" else v.tobytes()) for name in LINKED_KW for k, v in res[0][name].items()}


def _arrays(d):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in d.items()}


ANALYSES = {
    # name: (run, check against the restatement, the result as bytes)
    "prune": (_run_prune, _check_prune, lambda r: {"state": r[0].tobytes()}),
    "decay": (_run_decay, _check_decay, lambda r: _arrays(r[0])),
    "blocks": (_run_blocks, _check_blocks, lambda r: {"sites": r[0].tobytes(), **{f"text_{f}": r[2][f] for f in ALL4},
                                                      **{f"values_{f}": r[1][f][0].tobytes() for f in ALL4},
                                                      **{f"present_{f}": r[1][f][1].tobytes() for f in ALL4}}),
    "site_ld": (_run_site_ld, _check_site_ld, lambda r: _arrays(r[0])),
    "clusters": (_run_clusters, _check_clusters, lambda r: {"ids": r[0].tobytes(), **_arrays(r[1])}),
    "grid": (_run_grid, _check_grid, lambda r: _arrays(r[0])),
    "linked": (_run_linked, _check_linked, _linked_bytes),
}


def _all(s, head):
    """Every analysis on s, each held to its restatement; returns {analysis: (bytes, stats)}."""
    out = {}
    for name, (run, check, as_bytes) in ANALYSES.items():
        res = run(s)
        print(f"{head} {check(s, res)}")
        out[name] = (as_bytes(res), res[-1])
    return out


# ---- one engine per case: the TSV and the seven analyses share it, as the binary's runs share a context ----
class Case(Sub):
    def __init__(self, name):
        self.name, self.mono = name, name.endswith("_mono")
        input_name, self.how, self.kernel, self.shape, self.span = CASES[name]
        inp = _input(input_name)
        eng = _new_engine(inp, self.how)
        try:
            self.planned = _plan(eng, inp)
            self.item_s1, self.item_count = _items(eng)
            super().__init__(eng, inp, _tsv(eng, inp))
        except BaseException:
            eng.close()
            raise


@pytest.fixture(scope="module")
def case(request):
    c = Case(request.param)
    yield c
    c.eng.close()


every_case = pytest.mark.parametrize("case", list(CASES), indirect=True)


@every_case
def test_family_shape_and_keys(case):
    """The kernel is the family's, in the dispatch table's shape; rows are several items long; the TSV's keys are the window's."""
    inp = case.inp
    assert case.eng.pair_kernel() == case.kernel
    assert capi.describe_dispatch(inp.n_ind, inp.masked) == case.shape
    assert os.environ.get("NGSLD_PAIR_KERNEL") is None
    per_row = np.bincount(case.item_s1)
    assert int(case.item_count.max()) == case.span and per_row.max() >= 3 and int(case.item_count.sum()) == len(inp.keys)
    rows = _rows(case.text)
    assert [tuple(ln.split("\t")[:3]) for ln in rows] == inp.key_columns()
    assert case.planned == len(inp.keys) == len(rows)
    ends = capi.window_ends(shard.pos_dist_from_positions(inp.chrs, inp.pos), len(inp.labels), max_kb_dist=WIN["max_kb_dist"])
    assert inp.keys == [(i, j) for i in range(len(ends)) for j in range(i + 1, int(ends[i]))]
    nan_rows = sum(1 for ln in rows if any("nan" in v for v in ln.split("\t")[3:7]))
    inf_rows = sum(1 for ln in rows if any("inf" in v for v in ln.split("\t")[3:7]))
    if case.mono:  # un-called monomorphic sites: non-finite rows, and pairs the replay settles on the device
        info = case.eng.replay_info()
        print(f"{case.name}: replay of the TSV run {info}")
        assert nan_rows > 0 and inf_rows > 0
        assert info["pairs_flagged"] > 0 and info["pairs_on_device"] > 0
    print(f"{case.name}: {case.kernel} ({case.shape}{', asked for with ' + case.how if case.how else ''}), {inp.n_ind} individuals"
          f"{' (a tenth without data, ignore_miss_data)' if inp.masked else ''}, pairs {len(rows)}, rows with nan {nan_rows}, with inf {inf_rows}, "
          f"items {len(case.item_count)} of up to {case.span} candidates, up to {per_row.max()} a row")


@every_case
@pytest.mark.parametrize("analysis", list(ANALYSES))
def test_analysis_equals_its_rule_on_own_tsv(case, analysis, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    run, check, _ = ANALYSES[analysis]
    res = run(case)
    info = case.eng.replay_info()  # (of the pass's last chunk of rows: here its only one)
    print(f"{case.name} ({case.kernel}, {case.shape}): {check(case, res)}")
    if case.mono:  # the record pass flagged pairs as printed, and the device replay settled them before the consumer read them
        print(f"{case.name}: replay under {analysis} {info}")
        assert info["pairs_flagged"] > 0 and info["pairs_on_device"] > 0
        if analysis == "site_ld":
            assert res[-1]["pairs_counted"] < res[-1]["pairs"]  # (the non-finite rows drop out)


@every_case  # (the same list as the other tests, so that a case's engine is made once; the cases not in SPOT_CASES return at once)
def test_rows_against_the_oracle(case):
    """Some 20 rows of the TSV against the oracle's own records of the two sites: D, D' and r2 as "%f" prints them.  A value
    the oracle puts on a "%f" tie (odd / 128) is no evidence either way: such a row is skipped, at most 2 of the 20."""
    if case.name not in SPOT_CASES:
        return
    inp = case.inp
    rows = _rows(case.text)
    index = {lab: k for k, lab in enumerate(inp.labels)}
    skipped = 0
    for k in sorted(np.random.default_rng(SPOT_SEED).choice(len(rows), SPOT_PAIRS, replace=False)):
        f = rows[k].split("\t")
        i, j = index[f[0]], index[f[1]]
        r = orc.Oracle(inp.raw[[i, j]], None, ignore_miss_data=inp.masked).run()[0]
        want = [float(r["D"]), float(r["Dp"]), float(r["r2"])]
        if printed_values.is_tie(np.array(want)).any():
            skipped += 1
            continue
        assert f[4:7] == [printed_values.printf_f(v) for v in want], (case.name, f[:3], f[4:7], want)
    print(f"{case.name}: {SPOT_PAIRS - skipped} rows equal the oracle's, {skipped} skipped on a tie")
    assert skipped <= 2


# ---- the same case cut small: other item and chunk shapes, the same bytes ----
CUTS = {
    # name: (case, pairs per item, chunks)
    "multi_items5": ("multi", 5, False),
    "multi-ab_items5": ("multi-ab", 5, False),
    "stream_items5": ("stream_resident", 5, False),
    "multi_chunks": ("multi", 16, True),
    "multi-ab_chunks": ("multi-ab", 16, True),
    "stream_chunks": ("stream_resident", 16, True),
    "multi-ab_items5_chunks": ("multi-ab", 5, True),
    # items of 5 candidates, seven of them per launch of every pass's kernel
    "stream_items5_slices7": ("stream_resident", 5, True, {"NGSLD_TEST_RECORD_SLICE_ITEMS": "7"}),
    # the linked text of every chunk from the host formatter: the device formatter's bytes
    "multi-ab_items5_host": ("multi-ab", 5, True, {"NGSLD_TEST_LINKED_FORCE_HOST": "1"}),
}


def _short_item_shapes(sub, items, span, head):
    """Where the linked rows and the grid's rows lie among items narrower than a wavefront (`items`: Engine.items() of the plan,
    in the table's order).  Every condition is one under which a fault in the placement of a survivor would change the bytes:

    * a linked row in an item shorter than the span (the `c < it.count` guard, a row's last item);
    * linked rows of one s1 in three items or more (row_off and byte_off carried over more than one item boundary of a row);
    * a survivor in an item's last candidate, count - 1;
    * a survivor in candidate 0 and a non-survivor between two survivors (the popcount below the lane and the scan of the lengths
      both skip a lane);
    * a cell of the grid with rows from two items of one s1 (the merge of a cell's lanes ends at the item: the cell is completed
      by atomics from two wavefronts)."""
    tab, inp = sub.table, sub.inp
    count = items["count"].astype(np.int64)
    assert (items["mask"] == (np.uint64(1) << items["count"].astype(np.uint64)) - np.uint64(1)).all()  # (no rnd_sample: every candidate)
    a, b = capi.items_to_pairs(items)
    assert np.array_equal(a, tab.s1) and np.array_equal(b, tab.s2)
    item_of = np.repeat(np.arange(len(items)), count)  # the item of row k of the table, and the row's candidate in it
    cand = tab.s2.astype(np.int64) - items["s2_begin"].astype(np.int64)[item_of]
    assert (0 <= cand).all() and (cand < count[item_of]).all()
    for name, kw in LINKED_KW.items():
        idx, _ = tab.want(**kw)
        it = item_of[idx]
        short = int((count[it] < span).sum())
        per_s1 = np.bincount(items["s1"][np.unique(it)])
        last = int((cand[idx] == count[it] - 1).sum())
        mask = np.zeros(len(items), dtype=np.uint64)
        np.bitwise_or.at(mask, it, np.uint64(1) << cand[idx].astype(np.uint64))
        # (bit 0 set and not 2^k - 1: a zero below the highest one)
        holes = int((((mask & np.uint64(1)) == 1) & ((mask & (mask + np.uint64(1))) != 0)).sum())
        print(f"{head} linked {name}: rows {len(idx)}, {short} in items shorter than {span}, up to {per_s1.max()} items with rows a site, "
              f"{last} rows in an item's last candidate, {holes} masks with candidate 0 and a hole")
        assert 0 < len(idx) < len(tab.rows)
        assert short > 0 and per_s1.max() >= 3 and last > 0 and holes > 0, name
    pos = np.asarray(inp.pos).astype(np.int64)
    k = np.flatnonzero(sub.grid_counted)
    # (a cell of one s1: the bin of s2; counted rows of one chromosome only)
    cell_item = np.unique(np.stack([tab.s1[k].astype(np.int64), pos[tab.s2[k].astype(np.int64)] // GRID_BIN, item_of[k]]), axis=1)
    _, per_cell = np.unique(cell_item[:2], axis=1, return_counts=True)
    print(f"{head} grid: {len(per_cell)} (site, cell) runs, {int((per_cell >= 2).sum())} of them with rows from two items or more")
    assert (per_cell >= 2).any()


@pytest.mark.parametrize("cut", list(CUTS))
def test_cut_small_gives_the_same_bytes(cut, monkeypatch):
    """pairs_per_item 5: items of 20 candidates under the multi-wavefront kernel and of 5 under the streaming kernel, no row a
    whole number of them, no item as wide as a wavefront.  Chunks: a tenth of the pairs a chunk (of the region's rows' pairs for
    the blocks), and the site-LD and grid passes once with their LDS tiles and once with global atomics.  Slices: seven items per
    launch of a pass's kernel.  The host formatter for the linked text.  Plan, TSV and every result keep their bytes, and the
    results are held to the restatements again.  (Pruning is cut in chunks too; its stats count none: see the module's text.)"""
    name, ppi, chunks, *more = CUTS[cut]
    extra = more[0] if more else {}
    input_name, how, kernel, _, span16 = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    inp = _input(input_name)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        n0 = _plan(eng, inp)
        text = _tsv(eng, inp)
        sub = Sub(eng, inp, text)  # (one for every pass: the table of the linked pairs is made once)
        base = _all(sub, f"{cut} default:")
        assert all(st["chunks"] == 1 for a, (_, st) in base.items() if a != "prune") and base["site_ld"][1]["lds"] == 1
        assert base["grid"][1]["lds"] == 1
        if ppi != 16:
            eng.set_tuning(pairs_per_item=ppi)
            assert _plan(eng, inp) == n0 == len(inp.keys)
            items = sub.items = eng.items()
            s1, count = items["s1"], items["count"]
            span = ppi * span16 // 16
            assert int(count.max()) == span < 64 and int(count.sum()) == n0 and np.bincount(s1).max() >= 64 // span
            assert (count < span).sum() > len(np.unique(s1)) // 2  # (most rows end in a shorter item: no multiples of the span)
            assert _tsv(eng, inp).encode() == text.encode()
            _short_item_shapes(sub, items, span, f"{cut} pairs_per_item {ppi}:")
        if chunks:
            for k in CHUNK_KNOBS:
                monkeypatch.setenv(k, str(n0 // 10))
            monkeypatch.setenv("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", str(inp.member_pairs // 10))
        for k, v in extra.items():
            monkeypatch.setenv(k, v)
        passes = [("LDS tiles", None)] + ([("global atomics", "0")] if chunks else [])
        for what, lds_bytes in passes:
            if lds_bytes is not None:
                monkeypatch.setenv("NGSLD_TEST_SITE_LDS_BYTES", lds_bytes)
                monkeypatch.setenv("NGSLD_TEST_GRID_LDS_BYTES", lds_bytes)
            got = _all(sub, f"{cut} pairs_per_item {ppi}{', small chunks' if chunks else ''}{''.join(f', {k}={v}' for k, v in extra.items())}, "
                            f"site LD and grid on {what}:")
            assert got["site_ld"][1]["lds"] == got["grid"][1]["lds"] == (1 if lds_bytes is None else 0)
            for a, (as_bytes, st) in got.items():
                assert as_bytes.keys() == base[a][0].keys()
                for k in as_bytes:
                    assert as_bytes[k] == base[a][0][k], (a, k)
                if a != "prune":
                    assert (st["chunks"] > 5) if chunks else (st["chunks"] == 1), (a, st["chunks"])
    finally:
        eng.close()
