"""Several analyses over one run of the pair kernels (ngsld_analyze, Engine.analyze, the binary with two or more analysis flags;
ANALYZE.md) against the single calls on a fresh engine over the same input.

The single calls' own rules are held by their own files (test_gpu_prune.py ... test_gpu_scan.py, test_gpu_analyses_by_family.py);
here every array a getter returns must have the single call's bytes -- doubles as int64 views, NaN in the same places --, every
pass's stats its fields but the milliseconds and `chunks`, and `pairs_run == pairs`: the pair kernels ran once.

The input is that of the analyses' family tests cut to 20 individuals: 400 sites on two chromosomes, a window of 20 kb (some
50,000 pairs, rows of up to 140), labels CHR:pos.  That is the smallest shape with several rows a chunk, both chromosomes in
one chunk and every pass non-empty.

GPU time of this file on one MI355X: see README.md (the tests row)."""
import ctypes as C
import filecmp
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
WIN = dict(max_kb_dist=20, extend_out=True)
NAMES = ("prune", "decay", "site_ld", "clusters", "grid", "scan")
KNOBS = ("NGSLD_TEST_ANALYZE_CHUNK_PAIRS", "NGSLD_TEST_RECORD_SLICE_ITEMS", "NGSLD_TEST_SUM_WRAP_LIMIT", "NGSLD_TEST_SCAN_PLANT_DP",
         "NGSLD_TEST_PRUNE_CHUNK_PAIRS", "NGSLD_TEST_DECAY_CHUNK_PAIRS", "NGSLD_TEST_SITE_CHUNK_PAIRS", "NGSLD_TEST_CLUSTER_CHUNK_PAIRS",
         "NGSLD_TEST_GRID_CHUNK_PAIRS", "NGSLD_TEST_SCAN_CHUNK_PAIRS")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---- inputs and settings ----
class Input:
    def __init__(self, n_sites, n_ind, seed, **skw):
        self.raw = synth.make_gl_numpy(n_sites, n_ind, seed, **{"depth": 4.0, **skw})
        self.chrs, self.pos = synth.make_positions(n_sites, 41, max_gap=300, n_chr=2)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(self.chrs, self.pos)]
        # the table's rows: every pair of the window, row by row (same chromosome, dist <= the limit)
        self.n_pairs = sum(1 for i in range(n_sites) for j in range(i + 1, n_sites)
                           if self.chrs[i] == self.chrs[j] and self.pos[j] - self.pos[i] <= 20_000)


@functools.lru_cache(maxsize=None)
def _input(name):
    if name == "uncalled_mono":  # un-called monomorphic sites at a decisive depth: pairs the exact-order replay settles
        return Input(300, 20, 1320, depth=30.0, mono_frac=0.3)
    if name == "family":         # the multi-wavefront kernel's cohort of tests/test_gpu_analyses_by_family.py
        import test_gpu_analyses_by_family as fam
        return fam._input("n1000")
    return Input(400, 20, 1320)


def _kw(inp, **over):
    """The keyword arguments of the six methods (all four statistics wherever a pass takes several)."""
    kw = dict(prune=dict(labels=inp.labels, min_weight=0.3, weight_type="a"),
              decay=dict(ld=ALL4, bin_size=33.3),
              site_ld=dict(ld=ALL4, abs_value=False, linked_min=0.3),
              clusters=dict(min_weight=0.3, min_size=1),
              grid=dict(labels=inp.labels, bin_size=2000, ld=ALL4, abs_value=False, linked_min=0.3),
              scan=dict(half_window=3000, ld=ALL4))
    kw.update(over)
    return kw


def _engine(inp, setting="plain"):
    """A planned context on the input.  setting: plain (un-called likelihoods), replay (the flagged pairs replayed on the device
    from the first one on), hard (--call_geno: the called-genotype kernel), family (the multi-wavefront kernel, items of 20)."""
    eng = capi.Engine(0)
    try:
        if setting == "replay":
            eng.set_exact_store(2)
        eng.set_geno_raw(inp.raw, **(dict(call_geno=(0.0, 0.0)) if setting == "hard" else {}))
        eng.set_pos_dist(shard.pos_dist_from_positions(inp.chrs, inp.pos))
        if setting == "family":
            eng.set_tuning(pairs_per_item=5)
        eng.planned = eng.plan(**WIN)
    except BaseException:
        eng.close()
        raise
    return eng


@functools.lru_cache(maxsize=None)
def _singles(input_name, setting):
    """The six single calls on a fresh engine, once per input and setting; nobody writes to what this returns."""
    inp = _input(input_name)
    kw = _kw(inp)
    eng = _engine(inp, setting)
    try:
        return {name: getattr(eng, name)(**kw[name]) for name in NAMES}
    finally:
        eng.close()


# ---- the comparison ----
def _same_array(got, want, where):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, where
    if want.dtype == np.float64:
        assert np.array_equal(np.isnan(got), np.isnan(want)), where
        ok = ~np.isnan(want)
        bad = np.nonzero(got[ok].view(np.int64) != want[ok].view(np.int64))[0]
        assert len(bad) == 0, (where, bad[:5], got[ok][bad[:5]], want[ok][bad[:5]])
    elif want.dtype.kind in "iu":
        assert got.tobytes() == want.tobytes(), where
    else:
        assert np.array_equal(got, want), where


def _same_result(name, got, want, cut=False):
    """What a method returns: arrays and dicts of arrays, then the stats.  cut: the list ran in other chunks and launches than
    the single call, so the clusters' count of launches follows the chunks and is left out as `chunks` is."""
    assert type(got) is type(want) and len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        if isinstance(w, dict):
            assert set(g) == set(w), (name, k)
            for key in w:
                _same_array(g[key], w[key], (name, key))
        else:
            _same_array(g, w, (name, k))
    gs, ws = got[-1], want[-1]
    assert set(gs) == set(ws), name
    for key in ws:
        if key.endswith("_ms") or key == "chunks" or (cut and key == "union_launches"):
            continue
        assert gs[key] == ws[key], (name, key, gs[key], ws[key])


def _same(results, want, names=NAMES, cut=False):
    assert tuple(results) == tuple(names)
    for name in names:
        _same_result(name, results[name], want[name], cut)


# ---- 1. all six in one call ----
def test_all_six_in_one_call_equal_the_single_calls():
    inp = _input("plain")
    want = _singles("plain", "plain")
    eng = _engine(inp)
    try:
        results, stats = eng.analyze(**_kw(inp))
    finally:
        eng.close()
    _same(results, want)
    assert stats["n_analyses"] == 6
    assert stats["pairs_run"] == stats["pairs"] == inp.n_pairs == eng.planned > 30_000
    assert stats["chunks"] == 1
    for name in NAMES:  # every pass non-empty, and the shared pair phase in every pass's stats
        assert results[name][-1]["pairs"] == inp.n_pairs and results[name][-1]["pairs_ms"] == stats["pairs_ms"] > 0
    assert results["prune"][-1]["edges"] > 0 and len(results["decay"][0]["n"]) > 10 and results["site_ld"][-1]["sites_with_pairs"] > 300
    assert results["clusters"][-1]["clusters_multi"] > 0 and results["grid"][-1]["cells"] > 10 and results["scan"][-1]["pairs_counted"] > 0
    assert len(set(inp.chrs)) == 2
    print(f"all six: {stats}")


# ---- 2. many chunks and many launches ----
def test_many_chunks_and_many_launches_give_the_same_bytes(monkeypatch):
    inp = _input("plain")
    want = _singles("plain", "plain")
    monkeypatch.setenv("NGSLD_TEST_ANALYZE_CHUNK_PAIRS", str(inp.n_pairs // 10))
    monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "7")
    # (the single calls' own chunk knobs are not read here)
    monkeypatch.setenv("NGSLD_TEST_SCAN_CHUNK_PAIRS", "1")
    monkeypatch.setenv("NGSLD_TEST_PRUNE_CHUNK_PAIRS", "1")
    eng = _engine(inp)
    try:
        results, stats = eng.analyze(**_kw(inp))
    finally:
        eng.close()
    _same(results, want, cut=True)
    assert stats["chunks"] >= 10 and stats["pairs_run"] == stats["pairs"] == inp.n_pairs
    assert results["clusters"][-1]["union_launches"] > 10 * stats["chunks"]  # (slices of 7 items: many launches a chunk)
    for name in NAMES:
        if "chunks" in results[name][-1]:
            assert results[name][-1]["chunks"] == stats["chunks"]
    print(f"cut: {stats}")


# ---- 3. other routes to the records ----
@pytest.mark.parametrize("input_name,setting", [("uncalled_mono", "replay"), ("plain", "hard"), ("family", "family")])
def test_other_routes_to_the_records(input_name, setting, monkeypatch):
    inp = _input(input_name)
    want = _singles(input_name, setting)
    if setting == "family":  # (more pairs a row here: still some ten chunks)
        monkeypatch.setenv("NGSLD_TEST_ANALYZE_CHUNK_PAIRS", str(len(inp.keys) // 10))
        monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "1000")
    eng = _engine(inp, setting)
    try:
        if setting == "hard":
            assert eng.pair_kernel() == "hard"
        if setting == "family":
            assert eng.pair_kernel() == "multi" and int(eng.items()["count"].max()) == 20
        results, stats = eng.analyze(**_kw(inp))
        info = eng.replay_info()
    finally:
        eng.close()
    _same(results, want, cut=setting == "family")
    assert stats["pairs_run"] == stats["pairs"] == eng.planned
    if setting == "replay":  # the records were flagged as printed and settled on the device before any pass read them
        assert info["pairs_flagged"] > 0 and info["pairs_on_device"] > 0, info
        assert results["site_ld"][-1]["pairs_counted"] < stats["pairs"]  # (non-finite rows drop out)
    print(f"{setting}: {stats} replay {info}")


# ---- 4. lists of one and of two ----
@pytest.mark.parametrize("name", NAMES)
def test_a_list_of_one_equals_its_single_call(name):
    inp = _input("plain")
    want = _singles("plain", "plain")
    eng = _engine(inp)
    try:
        results, stats = eng.analyze(**{name: _kw(inp)[name]})
    finally:
        eng.close()
    _same(results, want, (name,))
    assert stats["n_analyses"] == 1 and stats["pairs_run"] == stats["pairs"] == inp.n_pairs


def test_two_kinds_whose_filters_differ_each_equal_their_single():
    inp = _input("plain")
    decay_kw, scan_kw = dict(ld=("r2", "Dp"), bin_size=100, min_maf=0.1, max_kb_dist=10), dict(half_window=5000, ld=("D",))
    eng = _engine(inp)
    try:
        results, stats = eng.analyze(decay=decay_kw, scan=scan_kw)
        fresh = _engine(inp)
        try:
            want = dict(decay=fresh.decay(**decay_kw), scan=fresh.scan(**scan_kw))
        finally:
            fresh.close()
    finally:
        eng.close()
    _same(results, want, ("decay", "scan"))
    assert results["decay"][-1]["pairs_counted"] < results["scan"][-1]["pairs_counted"]  # (the maf filter and the limit bite)
    assert stats["n_analyses"] == 2 and stats["pairs_run"] == stats["pairs"]


# ---- 5. refusals, none of which starts the pair kernels ----
def _stores_empty(eng, names):
    """Every getter of the named kinds answers as before any call."""
    L, h = eng._L, eng._h
    n = C.c_uint64(99)
    if "decay" in names:
        assert L.ngsld_decay_bins(h, 0, None, None, None, C.byref(n)) == capi.OK and n.value == 0
    if "site_ld" in names:
        assert L.ngsld_site_ld_get(h, 7, None, None, None, None, None) == capi.ERR_INVALID
    if "clusters" in names:
        assert L.ngsld_clusters_sites(h, None) == capi.ERR_INVALID
        assert L.ngsld_clusters_table(h, 1, 0, None, None, None, None, None, None, None, None, None, C.byref(n)) == capi.ERR_INVALID
    if "grid" in names:
        assert L.ngsld_grid_cells(h, 0, None, None, None, None, C.byref(n)) == capi.ERR_INVALID
        assert L.ngsld_grid_get(h, 7, 0, None, None, None, None) == capi.ERR_INVALID
    if "scan" in names:
        assert L.ngsld_scan_get(h, 7, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID


def _raw_list(eng, jobs):
    arr = (capi.Analysis * max(len(jobs), 1))()
    for a, job in zip(arr, jobs):
        a.struct_size, a.kind = C.sizeof(capi.Analysis), job.kind
        a.params, a.stats = C.addressof(job.params), C.addressof(job.stats)
        if job.labels is not None:
            a.labels = C.cast(job.labels, C.POINTER(C.c_char_p))
        if job.site_state is not None:
            a.site_state = job.site_state.ctypes.data
    return arr


def test_refusals_before_the_pair_kernels_start():
    inp = _input("plain")
    want = _singles("plain", "plain")
    kw = _kw(inp)
    eng = _engine(inp)
    try:
        L, h = eng._L, eng._h
        site_before = eng.site_ld(**kw["site_ld"])  # a store of a kind that no refused list names
        st = capi.AnalyzeStats()
        st.struct_size = C.sizeof(capi.AnalyzeStats)

        def refused(arr, n, text):
            st.pairs_run = 99
            assert L.ngsld_analyze(h, arr, n, C.byref(st)) == capi.ERR_INVALID
            msg = L.ngsld_last_error(h).decode()
            assert text in msg, msg
            assert st.pairs_run == 0 and st.chunks == 0
            return msg

        # an empty list
        refused(None, 0, "empty")
        jobs = [eng._decay_job(**kw["decay"]), eng._scan_job(**kw["scan"])]
        refused(_raw_list(eng, jobs), 0, "empty")
        # a filled store of each listed kind, then: an unknown kind, a kind twice, a wrong struct_size
        for case in ("unknown", "twice", "size"):
            eng.analyze(decay=kw["decay"], scan=kw["scan"])
            jobs = [eng._decay_job(**kw["decay"]), eng._scan_job(**kw["scan"]), eng._decay_job(**kw["decay"])]
            arr = _raw_list(eng, jobs)
            if case == "unknown":
                arr[2].kind = 7
                refused(arr, 3, "unknown kind 7")
                arr[2].kind = 0
                refused(arr, 3, "unknown kind 0")
            elif case == "twice":
                refused(arr, 3, "listed twice")
            else:
                arr[2].kind = capi.AN_GRID
                arr[2].struct_size = C.sizeof(capi.Analysis) - 8
                refused(arr, 3, "struct_size")
            _stores_empty(eng, ("decay", "scan"))
        # a bad parameter in the last entry: the scan's half window beyond the plan's max_kb_dist, in ngsld_scan's own words
        eng.analyze(decay=kw["decay"], grid=kw["grid"])
        with pytest.raises(capi.NgsldError) as single:
            eng.scan(10001)
        with pytest.raises(capi.NgsldError) as e:
            eng.analyze(decay=kw["decay"], grid=kw["grid"], scan=dict(half_window=10001))
        assert e.value.code == capi.ERR_INVALID and e.value.msg == single.value.msg and "20002 bp" in e.value.msg
        assert eng.analyze_stats.pairs_run == 0
        _stores_empty(eng, ("decay", "grid", "scan"))
        # none of them started the pair kernels (the scan alone did, above: it is a single call's refusal before any device work)
        # and the store of the kind not listed is intact
        _site_store_is(eng, site_before[0])
        # the context stays usable
        results, stats = eng.analyze(**kw)
    finally:
        eng.close()
    _same(results, want)
    assert stats["pairs_run"] == stats["pairs"] == inp.n_pairs


def _site_store_is(eng, sites):
    """The context's site LD store, read through its getter, holds the arrays an earlier Engine.site_ld returned."""
    m = len(sites["n"])
    for k, f in enumerate(ALL4):
        n, mean = np.zeros(m, dtype=np.uint64), np.zeros(m)
        arrs = [np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.uint64)]
        assert eng._L.ngsld_site_ld_get(eng._h, 4 + k, n.ctypes.data, *(a.ctypes.data for a in arrs), mean.ctypes.data) == capi.OK
        for got, key in zip([n, *arrs, mean], ("n", f"sum_{f}", f"max_{f}", f"linked_{f}", f"mean_{f}")):
            _same_array(got, sites[key], key)


# ---- 6. refusals that arrive mid-run ----
def test_a_planted_value_in_a_late_chunk_fails_with_the_scans_message_and_empties_every_store(monkeypatch):
    inp = _input("plain")
    want = _singles("plain", "plain")
    kw = _kw(inp)
    eng = _engine(inp)
    try:
        # record `at` of the plan: in a late chunk, every field finite (the scan reads it) and not a row's first candidate
        s1, s2, std, _ = eng.run()
        at = next(k for k in range(inp.n_pairs * 3 // 4, inp.n_pairs)
                  if all(math.isfinite(float(std[f][k])) for f in ALL4) and s2[k] > s1[k] + 1)
        site_before = eng.site_ld(**kw["site_ld"])
        monkeypatch.setenv("NGSLD_TEST_ANALYZE_CHUNK_PAIRS", str(inp.n_pairs // 10))
        monkeypatch.setenv("NGSLD_TEST_SCAN_PLANT_DP", f"{at}:274877.906944")
        with pytest.raises(capi.NgsldError) as e:
            eng.analyze(prune=kw["prune"], decay=kw["decay"], clusters=kw["clusters"], grid=kw["grid"], scan=kw["scan"])
        assert e.value.code == capi.ERR_UNSUPPORTED, e.value.msg
        assert f"a scan value of the pair of sites {int(s1[at])} - {int(s2[at])} reaches 2^38 micro-units" in e.value.msg, e.value.msg
        st = eng.analyze_stats
        assert 0 < st.pairs_run < st.pairs == inp.n_pairs and st.chunks >= 7  # (decay's chunks had run)
        _stores_empty(eng, ("decay", "clusters", "grid", "scan"))
        _site_store_is(eng, site_before[0])  # (not listed: intact)
        monkeypatch.delenv("NGSLD_TEST_SCAN_PLANT_DP")
        results, stats = eng.analyze(**kw)
    finally:
        eng.close()
    _same(results, want, cut=True)
    assert stats["chunks"] >= 10


def test_the_sum_guard_pinned_to_the_unit_gives_the_singles_refusal(monkeypatch):
    """NGSLD_TEST_SUM_WRAP_LIMIT = 1 turns every pass's tracking of max |q| on and refuses any sum that holds a value: the list
    fails with the message of the single call of the first listed pass that sums (pruning does not)."""
    inp = _input("plain")
    kw = _kw(inp)
    monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", "1")
    eng = _engine(inp)
    try:
        for first, others in (("site_ld", ("prune",)), ("decay", ("scan",)), ("scan", ("prune",)), ("grid", ()), ("clusters", ("prune",))):
            with pytest.raises(capi.NgsldError) as single:
                getattr(eng, first)(**kw[first])
            assert single.value.code == capi.ERR_UNSUPPORTED and "too large to sum exactly" in single.value.msg
            names = [n for n in NAMES if n == first or n in others]
            with pytest.raises(capi.NgsldError) as e:
                eng.analyze(**{n: kw[n] for n in names})
            assert e.value.code == capi.ERR_UNSUPPORTED and e.value.msg == single.value.msg, (first, e.value.msg, single.value.msg)
            _stores_empty(eng, names)
        monkeypatch.delenv("NGSLD_TEST_SUM_WRAP_LIMIT")
        results, _ = eng.analyze(site_ld=kw["site_ld"])
    finally:
        eng.close()
    _same(results, _singles("plain", "plain"), ("site_ld",))


def test_a_chunk_below_the_longest_row_is_refused_with_pruning_listed_only(monkeypatch):
    inp = _input("plain")
    want = _singles("plain", "plain")
    kw = _kw(inp)
    monkeypatch.setenv("NGSLD_TEST_ANALYZE_CHUNK_PAIRS", "50")
    eng = _engine(inp)
    try:
        row_off, _ = eng.plan_rows()
        longest = int(np.diff(row_off).max())
        assert longest > 100
        monkeypatch.setenv("NGSLD_TEST_PRUNE_CHUNK_PAIRS", "50")
        with pytest.raises(capi.NgsldError) as single:
            eng.prune(**kw["prune"])
        monkeypatch.delenv("NGSLD_TEST_PRUNE_CHUNK_PAIRS")
        with pytest.raises(capi.NgsldError) as e:
            eng.analyze(prune=kw["prune"], decay=kw["decay"])
        assert e.value.code == capi.ERR_UNSUPPORTED and e.value.msg == single.value.msg and "does not fit the record buffer" in e.value.msg
        _stores_empty(eng, ("decay",))
        results, stats = eng.analyze(decay=kw["decay"], scan=kw["scan"])  # (the context stays usable; the buffer fits the row)
    finally:
        eng.close()
    _same(results, want, ("decay", "scan"))
    assert stats["pairs_run"] == stats["pairs"] and stats["chunks"] > 100


# ---- 7. the binary ----
def test_cli_one_invocation_writes_the_files_of_six(tmp_path):
    inp = _input("plain")
    n_sites, n_ind = inp.raw.shape[0], inp.raw.shape[1]
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    inp.raw.astype("<f8").tofile(g)
    synth.write_pos(p, inp.chrs, inp.pos)
    common = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "20", "--extend_out", "--pos", p]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}

    def run(*a):
        r = subprocess.run([*common, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return r

    def flags(tag):
        return {"prune": ["--prune_out", f"{tag}_kept.txt", "--prune_excl", f"{tag}_excl.txt", "--prune_min_weight", "0.3"],
                "decay": ["--decay_out", f"{tag}_decay.tsv", "--decay_fit", f"{tag}_fit.tsv", "--decay_ld", "r2,Dp", "--decay_bin_size", "100"],
                "site": ["--site_out", f"{tag}_site.tsv", "--site_ld", "r2,D", "--site_signed"],
                "cluster": ["--cluster_out", f"{tag}_cl.tsv", "--cluster_table", f"{tag}_clt.tsv", "--cluster_min_weight", "0.3"],
                "grid": ["--grid_out", f"{tag}_grid.tsv", "--grid_bin_size", "2000", "--grid_ld", "r2,Dp"],
                "scan": ["--scan_out", f"{tag}_scan.tsv", "--scan_half_window", "3000", "--scan_ld", "r2,Dp"]}

    files = ("kept.txt", "excl.txt", "decay.tsv", "fit.tsv", "site.tsv", "cl.tsv", "clt.tsv", "grid.tsv", "scan.tsv")
    r = run(*[x for fl in flags("all").values() for x in fl])
    assert f"==> analyses: 6 share one run of {inp.n_pairs} pairs in 1 chunks\n" in r.stderr, r.stderr[-2000:]
    for fl in flags("one").values():
        r1 = run(*fl)
        assert "==> analyses:" not in r1.stderr
    for f in files:
        assert os.path.getsize(tmp_path / f"one_{f}") > 0, f
        assert filecmp.cmp(tmp_path / f"all_{f}", tmp_path / f"one_{f}", shallow=False), f
    # --out beside two analyses: the table is that of --out alone
    r = run("--out", "t2.tsv", *flags("two")["decay"], *flags("two")["scan"])
    assert "==> analyses: 2 share one run of " in r.stderr
    run("--out", "t0.tsv")
    assert filecmp.cmp(tmp_path / "t2.tsv", tmp_path / "t0.tsv", shallow=False) and os.path.getsize(tmp_path / "t0.tsv") > 100_000
    for f in ("decay.tsv", "fit.tsv", "scan.tsv"):
        assert filecmp.cmp(tmp_path / f"two_{f}", tmp_path / f"one_{f}", shallow=False), f


def test_cli_blocks_beside_a_bundle_leave_its_results_alone(tmp_path):
    """--blocks_out beside two bundled families and no --out: ngsld_blocks runs between ngsld_analyze and the families' writers
    (blocks come first in the families' order) and must not empty what the bundle left for them."""
    inp = _input("plain")
    n_sites, n_ind = inp.raw.shape[0], inp.raw.shape[1]
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    inp.raw.astype("<f8").tofile(g)
    synth.write_pos(p, inp.chrs, inp.pos)
    common = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "20", "--extend_out", "--pos", p]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}

    def flags(tag):
        return {"site": ["--site_out", f"{tag}_site.tsv", "--site_ld", "r2,D", "--site_signed"],
                "grid": ["--grid_out", f"{tag}_grid.tsv", "--grid_bin_size", "2000", "--grid_ld", "r2,Dp"],
                "blocks": ["--blocks_out", f"{tag}_B", "--blocks_chr", inp.chrs[40], "--blocks_start", str(int(inp.pos[40])),
                           "--blocks_end", str(int(inp.pos[60]))]}

    def run(*a):
        return subprocess.run([*common, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)

    r = run(*[x for fl in flags("all").values() for x in fl])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "==> analyses: 2 share one run of " in r.stderr and r.stdout == ""
    for fl in flags("one").values():
        r1 = run(*fl)
        assert r1.returncode == 0, r1.stderr[-2000:]
    for f in ("site.tsv", "grid.tsv", "B.r2.tsv", "B.Dp.tsv"):
        assert os.path.getsize(tmp_path / f"one_{f}") > 100, f
        assert filecmp.cmp(tmp_path / f"all_{f}", tmp_path / f"one_{f}", shallow=False), f
