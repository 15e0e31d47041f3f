"""The five record passes -- LD pruning, decay, blocks, site LD and clusters -- under every pair-kernel family.

The five analyses' own files hold each pass, bit for bit, to its plain-Python rule (prune_ref, decay_ref, blocks_ref, site_ref,
cluster_ref) applied to the engine's own TSV, on cohorts of 4 to 500 individuals: the 8-lane group kernel, the run kernel at 8
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

GPU time of this file on one MI355X: see README.md (the tests row)."""
import functools
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
from test_gpu_site_ld import _same as _same_site_ld

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
WIN = dict(max_kb_dist=20, extend_out=True)
LIMIT = 20_000
PRUNE_KW = dict(min_weight=0.3, weight_type="a")  # (test_gpu_prune.py's floor from 500 individuals on)
DECAY_KW = dict(ld=ALL4, bin_size=33.3)
SITE_KW = dict(ld=ALL4, abs_value=False, linked_min=0.3)
CHUNK_KNOBS = ("NGSLD_TEST_DECAY_CHUNK_PAIRS", "NGSLD_TEST_SITE_CHUNK_PAIRS", "NGSLD_TEST_CLUSTER_CHUNK_PAIRS",
               "NGSLD_TEST_PRUNE_CHUNK_PAIRS")
KNOBS = CHUNK_KNOBS + ("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", "NGSLD_TEST_SITE_LDS_BYTES", "NGSLD_TEST_DECAY_LDS_BYTES",
                       "NGSLD_TEST_BLOCKS_HOST_ROWS", "NGSLD_TEST_BLOCKS_TEXT_ROWS")
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


class Sub:
    """An engine with its plan, its input and its own TSV: what an analysis is run on and checked against."""

    def __init__(self, eng, inp, text):
        self.eng, self.inp, self.text = eng, inp, text
        self.labels = tuple(inp.labels)
        self.n_pairs = len(inp.keys)

    @property
    def floor(self):
        return _want(self.text, self.labels, "floor")


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
    assert stats["union_launches"] == stats["chunks"]
    return (f"clusters: floor {s.floor} pairs {stats['pairs']} nodes {stats['nodes']} edges {stats['edges']} clusters {stats['clusters']} "
            f"largest {stats['largest']} chunks {stats['chunks']}")


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
}


def _all(s, head):
    """Every analysis on s, each held to its restatement; returns {analysis: (bytes, stats)}."""
    out = {}
    for name, (run, check, as_bytes) in ANALYSES.items():
        res = run(s)
        print(f"{head} {check(s, res)}")
        out[name] = (as_bytes(res), res[-1])
    return out


# ---- one engine per case: the TSV and the five analyses share it, as the binary's runs share a context ----
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
}


@pytest.mark.parametrize("cut", list(CUTS))
def test_cut_small_gives_the_same_bytes(cut, monkeypatch):
    """pairs_per_item 5: items of 20 candidates under the multi-wavefront kernel and of 5 under the streaming kernel, no row a
    whole number of them, no item as wide as a wavefront.  Chunks: a tenth of the pairs a chunk (of the region's rows' pairs for
    the blocks), and the site-LD pass once with its LDS tiles and once with global atomics.  Plan, TSV and every result keep
    their bytes, and the results are held to the restatements again.  (Pruning is cut in chunks too; its stats count none: see the
    module's text.)"""
    name, ppi, chunks = CUTS[cut]
    input_name, how, kernel, _, span16 = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    inp = _input(input_name)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        n0 = _plan(eng, inp)
        text = _tsv(eng, inp)
        base = _all(Sub(eng, inp, text), f"{cut} default:")
        assert all(st["chunks"] == 1 for a, (_, st) in base.items() if a != "prune") and base["site_ld"][1]["lds"] == 1
        if ppi != 16:
            eng.set_tuning(pairs_per_item=ppi)
            assert _plan(eng, inp) == n0 == len(inp.keys)
            s1, count = _items(eng)
            span = ppi * span16 // 16
            assert int(count.max()) == span < 64 and int(count.sum()) == n0 and np.bincount(s1).max() >= 64 // span
            assert (count < span).sum() > len(np.unique(s1)) // 2  # (most rows end in a shorter item: no multiples of the span)
            assert _tsv(eng, inp).encode() == text.encode()
        if chunks:
            for k in CHUNK_KNOBS:
                monkeypatch.setenv(k, str(n0 // 10))
            monkeypatch.setenv("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", str(inp.member_pairs // 10))
        passes = [("LDS tiles", None)] + ([("global atomics", "0")] if chunks else [])
        for what, lds_bytes in passes:
            if lds_bytes is not None:
                monkeypatch.setenv("NGSLD_TEST_SITE_LDS_BYTES", lds_bytes)
            got = _all(Sub(eng, inp, text), f"{cut} pairs_per_item {ppi}{', small chunks' if chunks else ''}, site LD on {what}:")
            assert got["site_ld"][1]["lds"] == (1 if lds_bytes is None else 0)
            for a, (as_bytes, st) in got.items():
                assert as_bytes.keys() == base[a][0].keys()
                for k in as_bytes:
                    assert as_bytes[k] == base[a][0][k], (a, k)
                if a != "prune":
                    assert (st["chunks"] > 5) if chunks else (st["chunks"] == 1), (a, st["chunks"])
    finally:
        eng.close()
