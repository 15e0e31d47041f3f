"""The LD scan on the device (ngsld_scan, Engine.scan, the binary's --scan_* flags) against tests/scan_ref.py -- the rule of
SCAN.md in plain Python -- applied to the same engine's own TSV (run_text).  Every window end, count and sum of every site must be
equal as integers and every zns and omega bit for bit: nothing sampled, no tolerance.

A value of 2^38 micro-units or more comes from no input (D' is a ratio of valid haplotype frequencies: the CPU oracle's largest
finite |D'| over the generator's settings is 1.64), so that refusal is reached with a value planted in one record through
NGSLD_TEST_SCAN_PLANT_DP.

GPU time of this file on one MI355X: see README.md (the tests row)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import scan_ref
from ngsld_amd import capi, shard, synth
from oracle import orc

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
KNOBS = ("NGSLD_TEST_SCAN_CHUNK_PAIRS", "NGSLD_TEST_RECORD_SLICE_ITEMS", "NGSLD_TEST_SUM_WRAP_LIMIT", "NGSLD_TEST_SCAN_PLANT_DP")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _names(n):
    """Labels that stay unique where two sites share a position; the windows come from (chrs, pos)."""
    return [f"s{k}" for k in range(n)]


def _tsv(eng, labels):
    eng.set_text_output(labels)
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _n_rows(text):
    return sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))


def _same(win, want, ld):
    chosen = [f for f in scan_ref.FIELDS if f in ld]
    keys = {"win_first", "win_last", "n_ll", "n_rr", "n_lr"} | {f"{w}_{f}" for f in chosen for w in ("sum_ll", "sum_rr", "sum_lr", "zns", "omega")}
    assert set(win) == keys
    for k in sorted(keys):
        if k.startswith(("zns_", "omega_")):
            exp = np.array([math.nan if x is None else x for x in want[k]])
            got = win[k]
            assert np.array_equal(np.isnan(got), np.isnan(exp)), k
            ok = ~np.isnan(exp)
            bad = np.nonzero(got[ok].view(np.int64) != exp[ok].view(np.int64))[0]
            assert len(bad) == 0, (k, bad[:5], got[ok][bad[:5]], exp[ok][bad[:5]])
        else:
            assert [int(x) for x in win[k]] == want[k], k


def _check(eng, text, labels, where, half, rows=None, **kw):
    """One Engine.scan held to the rule on `text`; rows: counted_rows of the same text and filters."""
    win, stats = eng.scan(half, **kw)
    want = scan_ref.scan(text, labels, half, positions=where, rows=rows, **kw)
    _same(win, want, kw.get("ld", ("r2",)))
    counted = len(rows) if rows is not None else len(scan_ref.counted_rows(text, labels, **kw))
    assert stats["pairs"] == _n_rows(text) and stats["pairs_counted"] == counted
    assert stats["largest_window"] == max(b - a + 1 for a, b in zip(want["win_first"], want["win_last"]))
    print(f"H {half}: pairs {stats['pairs']} counted {stats['pairs_counted']} largest window {stats['largest_window']} chunks {stats['chunks']} "
          f"pairs_ms {stats['pairs_ms']:.2f} scan_ms {stats['scan_ms']:.3f} total_ms {stats['total_ms']:.2f}")
    return win, stats, want


def _positions(n_sites, seed, max_gap, n_chr, zero_gaps=0):
    """synth.make_positions, with `zero_gaps` sites moved onto their left neighbour's position (never a chromosome's first)."""
    chrs, pos = synth.make_positions(n_sites, seed, max_gap=max_gap, n_chr=n_chr)
    pos = pos.copy()
    rng = np.random.default_rng(seed)
    for k in sorted(rng.choice(np.arange(1, n_sites), size=zero_gaps, replace=False)):
        if chrs[k] == chrs[k - 1]:
            pos[k] = pos[k - 1]
    assert all(chrs[k] != chrs[k - 1] or pos[k] >= pos[k - 1] for k in range(1, n_sites))
    return chrs, pos


# ---- windowed runs: 600 sites x 20 individuals, two chromosomes, some sites on one position, a plan window of 20 kb ----
@functools.lru_cache(maxsize=1)
def _windowed():
    n_sites = 600
    raw = synth.make_gl_numpy(n_sites, 20, 620, depth=4.0)
    chrs, pos = _positions(n_sites, 43, 500, 2, zero_gaps=40)
    return raw, chrs, pos, list(zip(chrs, (int(p) for p in pos)))


@functools.lru_cache(maxsize=1)
def _windowed_table():
    """The engine's TSV of the windowed input and its counted rows with all four statistics, once."""
    raw, chrs, pos, where = _windowed()
    labels = _names(len(chrs))
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        text = _tsv(eng, labels)
    finally:
        eng.close()
    return text, labels, scan_ref.counted_rows(text, labels, ld=ALL4)


def test_windowed_runs_at_three_half_windows():
    raw, chrs, pos, where = _windowed()
    text, labels, rows = _windowed_table()
    assert sum(1 for k in range(1, len(pos)) if chrs[k] == chrs[k - 1] and pos[k] == pos[k - 1]) >= 30
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        items = eng.items()
        per_row = np.bincount(items["s1"].astype(np.int64), minlength=len(chrs))
        assert per_row.max() >= 2 and int(items["count"].max()) == 64  # (rows longer than 64 candidates: several items a row)
        seen = set()
        for half in (500, 3000, 10000):
            _, stats, want = _check(eng, text, labels, where, half, rows=rows, ld=ALL4)
            a, b = want["win_first"], want["win_last"]
            for k in ("n_ll", "n_rr", "n_lr"):
                if any(want[k]):
                    seen.add(k)
            if half == 500:  # a_j > i inside a row's first item: the RR range is empty there, the LR range begins at a_j
                assert any(a[j] > i for i, j, _ in rows if j - i < 64)
            if half == 10000:  # the window reaches the plan's: rows 2 H apart exist and are in no flank
                assert max(b[c] - a[c] for c in range(len(a))) > 64
                assert max(pos[j] - pos[i] for i, j, _ in rows) > 19000
        assert seen == {"n_ll", "n_rr", "n_lr"}
    finally:
        eng.close()


def test_a_half_window_beyond_the_plan_is_refused_and_the_context_stays_usable():
    raw, chrs, pos, where = _windowed()
    text, labels, rows = _windowed_table()
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        with pytest.raises(capi.NgsldError) as e:
            eng.scan(10001)
        assert e.value.code == capi.ERR_INVALID and "20002 bp" in e.value.msg and "20000 bp" in e.value.msg and "10001" in e.value.msg
        n = np.zeros(len(chrs), dtype=np.uint64)
        assert eng._L.ngsld_scan_get(eng._h, 7, None, None, n.ctypes.data, None, None, None, None, None, None, None) == capi.ERR_INVALID
        r2_rows = scan_ref.counted_rows(text, labels)
        win, _, _ = _check(eng, text, labels, where, 10000, rows=r2_rows)
        assert eng._L.ngsld_scan_get(eng._h, 7, None, None, n.ctypes.data, None, None, None, None, None, None, None) == capi.OK
        assert n.tobytes() == win["n_ll"].tobytes()
        assert eng._L.ngsld_scan_get(eng._h, 5, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID  # (D not chosen)
        eng.plan(max_kb_dist=20, extend_out=True)  # (the result goes with the plan)
        assert eng._L.ngsld_scan_get(eng._h, 7, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
        with pytest.raises(capi.NgsldError) as e:
            eng.scan(2 ** 31)
        assert e.value.code == capi.ERR_INVALID and "2^31" in e.value.msg
    finally:
        eng.close()


def test_refusals_of_the_entry():
    raw = synth.make_gl_numpy(100, 16, 3, depth=4.0)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(np.full(100, 10.5))  # (positions no file holds: half a base between sites)
        eng.plan(max_kb_dist=1, extend_out=True)
        with pytest.raises(capi.NgsldError) as e:
            eng.scan(100)
        assert e.value.code == capi.ERR_UNSUPPORTED and "integer position gaps" in e.value.msg
        import ctypes as C
        p = capi.ScanParams(C.sizeof(capi.ScanParams) - 8, 8, 100, math.inf, 0.0, 0)
        assert eng._L.ngsld_scan(eng._h, C.byref(p), None) == capi.ERR_INVALID
        assert b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = capi.ScanParams(C.sizeof(capi.ScanParams), 16, 100, math.inf, 0.0, 0)
        assert eng._L.ngsld_scan(eng._h, C.byref(p), None) == capi.ERR_INVALID
        p = capi.ScanParams(C.sizeof(capi.ScanParams), 8, 100, math.nan, 0.0, 0)
        assert eng._L.ngsld_scan(eng._h, C.byref(p), None) == capi.ERR_INVALID
    finally:
        eng.close()


def test_all_pairs_and_a_half_window_beyond_the_chromosome():
    """No window in the plan, H beyond either chromosome: every row of a chromosome is in every window of it, and the rows across
    the two chromosomes (dist inf) are counted nowhere."""
    raw = synth.make_gl_numpy(300, 64, 864, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300, n_chr=2)
    where, labels = list(zip(chrs, (int(p) for p in pos))), _names(300)
    eng = _engine(raw, chrs, pos, dict(extend_out=True))
    try:
        text = _tsv(eng, labels)
        win, stats, want = _check(eng, text, labels, where, 10 ** 9, ld=ALL4)
    finally:
        eng.close()
    per_chr = 150 * 149 // 2
    assert stats["pairs"] == 300 * 299 // 2 and stats["pairs_counted"] == 2 * per_chr and stats["largest_window"] == 150
    assert [int(x) for x in win["n_ll"] + win["n_rr"] + win["n_lr"]] == [per_chr] * 300
    assert len({float(x) for x in win["zns_r2"][:150]}) == 1 and len({float(x) for x in win["zns_r2"][150:]}) == 1


# ---- dropped rows and degenerate values ----
DROP_CASES = {
    # name: (n_ind, synth kw, plan kw, geno kw, scan kw, half window)
    "uncalled_mono": (20, dict(mono_frac=0.2, depth=60.0), dict(max_kb_dist=20, extend_out=True), None, dict(ld=ALL4), 4000),
    "call_geno": (64, dict(depth=4.0), dict(max_kb_dist=20, extend_out=True), dict(call_geno=(0.1, 0.9)), dict(ld=("r2", "Dp")), 4000),
    "rnd_sample": (20, dict(depth=4.0), dict(max_kb_dist=20, rnd_sample=0.5, seed=7, extend_out=True), None, dict(ld=("D", "r2")), 4000),
    "min_maf_and_kb_inside": (64, dict(depth=4.0), dict(max_kb_dist=20, extend_out=True), None,
                              dict(ld=("r2_ExpG", "r2"), min_maf=0.2, max_kb_dist=7.5), 6000),
}


@pytest.mark.parametrize("name", list(DROP_CASES))
def test_dropped_rows(name):
    n_ind, skw, plan_kw, geno_kw, scan_kw, half = DROP_CASES[name]
    n_sites = 400
    raw = synth.make_gl_numpy(n_sites, n_ind, 700 + n_ind, **skw)
    chrs, pos = _positions(n_sites, 47, 300, 2, zero_gaps=10)
    where, labels = list(zip(chrs, (int(p) for p in pos))), _names(n_sites)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, labels)
        win, stats, want = _check(eng, text, labels, where, half, **scan_kw)
        items = eng.items()
    finally:
        eng.close()
    assert 0 < stats["pairs_counted"] and int(win["n_lr"].sum()) > 0 and int(win["n_ll"].sum()) > 0 and int(win["n_rr"].sum()) > 0
    if name == "uncalled_mono":
        assert ("nan" in text or "inf" in text) and stats["pairs_counted"] < stats["pairs"]  # (NaN / inf rows drop out)
    if name == "rnd_sample":  # (masks with holes: a candidate that was not drawn between two that were)
        assert any(bin(int(m)).count("1") < int(m).bit_length() for m in items["mask"])
    if name == "min_maf_and_kb_inside":
        assert stats["pairs_counted"] < len(scan_ref.counted_rows(text, labels, ld=scan_kw["ld"], max_kb_dist=7.5)) \
            < len(scan_ref.counted_rows(text, labels, ld=scan_kw["ld"]))


def test_omega_is_na_where_every_row_across_prints_zero():
    """Called genotypes of 8 individuals at sites drawn independently (p_resample 1: neighbours are not in LD): one r2 in twelve
    prints as 0.000000.  With a window of a few sites some site's rows across it all do: S_LR == 0 with n_LR > 0, omega NA beside
    a zns of its own and rows inside a flank.  That the input holds such a site is checked on the CPU first, through the oracle's
    records of the same pairs."""
    n_sites, half = 300, 150
    raw = np.eye(3)[synth.make_gl_numpy(n_sites, 8, 16, depth=8.0, p_resample=1.0).argmax(2)]
    chrs, pos = synth.make_positions(n_sites, 48, max_gap=300)
    pd = shard.pos_dist_from_positions(chrs, pos)
    where, labels = list(zip(chrs, (int(p) for p in pos))), _names(n_sites)
    rec = orc.Oracle(raw, pd, max_kb_dist=5, n_threads=8).run()
    a, b = scan_ref.windows(where, n_sites, half)
    rows = [(int(r["s1"]), int(r["s2"]), (abs(scan_ref.micro("%f" % r["r2"])),)) for r in rec if math.isfinite(r["r2"])]
    cpu = scan_ref.scan_rows(rows, a, b, ["r2"])
    sites = [c for c in range(n_sites) if cpu["n_lr"][c] > 0 and cpu["sum_lr_r2"][c] == 0 and cpu["n_ll"][c] + cpu["n_rr"][c] > 0]
    assert sites, "the input has no site whose rows across it all print 0.000000"
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=5, extend_out=True))
    try:
        text = _tsv(eng, labels)
        win, _, want = _check(eng, text, labels, where, half)
    finally:
        eng.close()
    for c in sites:
        assert want["n_lr"][c] > 0 and want["sum_lr_r2"][c] == 0 and math.isnan(win["omega_r2"][c]) and not math.isnan(win["zns_r2"][c])
    print(f"{len(sites)} sites with rows across them that all print 0.000000, e.g. site {sites[0]}")


# ---- cuts: chunks of a tenth of the pairs, launches of 7 items ----
def test_chunks_and_slices_give_the_bytes_of_the_uncut_call(monkeypatch):
    raw, chrs, pos, where = _windowed()
    text, labels, rows = _windowed_table()
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        base, s0, _ = _check(eng, text, labels, where, 3000, rows=rows, ld=ALL4)
        assert s0["chunks"] == 1
        monkeypatch.setenv("NGSLD_TEST_SCAN_CHUNK_PAIRS", str(s0["pairs"] // 10))
        monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "7")
        cut, s1 = eng.scan(3000, ld=ALL4)
        assert s1["chunks"] > 1 and s1["pairs_counted"] == s0["pairs_counted"]
        monkeypatch.delenv("NGSLD_TEST_RECORD_SLICE_ITEMS")
        chunked, s2 = eng.scan(3000, ld=ALL4)
        assert s2["chunks"] == s1["chunks"]
    finally:
        eng.close()
    for got in (cut, chunked):
        assert got.keys() == base.keys()
        for k in base:
            assert got[k].tobytes() == base[k].tobytes(), k


# ---- the guard of the integer sums ----
@pytest.mark.parametrize("cut", [False, True])
def test_sum_guard_is_pinned_to_the_unit(cut, monkeypatch):
    """NGSLD_TEST_SUM_WRAP_LIMIT = L turns the tracking of max |q| on and puts the limit at L: with M the largest |q| of a counted
    row and N = C(largest window, 2) the rows a window can hold, L = M N + 1 passes and L = M N is refused."""
    raw, chrs, pos, where = _windowed()
    text, labels, _ = _windowed_table()
    half, ld = 3000, ("D",)  # (|D| has one largest value in one pair or two; D' and r2 print 1.000000 in many)
    rows = scan_ref.counted_rows(text, labels, ld=ld)
    a, b = scan_ref.windows(where, len(labels), half)
    m = max(y - x + 1 for x, y in zip(a, b))
    N, M = m * (m - 1) // 2, max(qs[0] for _, _, qs in rows)
    holders = [(i, j) for i, j, qs in rows if qs[0] == M]
    assert M > 0 and M * N < 2 ** 63 and m > 20
    if cut:
        monkeypatch.setenv("NGSLD_TEST_SCAN_CHUNK_PAIRS", str(_n_rows(text) // 10))
        monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "7")
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(M * N + 1))
        base, st, _ = _check(eng, text, labels, where, half, rows=rows, ld=ld)
        assert (st["chunks"] > 1) == cut
        monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(M * N))
        with pytest.raises(capi.NgsldError) as e:
            eng.scan(half, ld=ld)
        assert e.value.code == capi.ERR_UNSUPPORTED and f"a window of up to {N} pairs" in e.value.msg and "too large to sum exactly" in e.value.msg
        assert eng._L.ngsld_scan_get(eng._h, 5, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
        monkeypatch.delenv("NGSLD_TEST_SUM_WRAP_LIMIT")
        again, _ = eng.scan(half, ld=ld)  # (the context stays usable, un-knobbed bytes)
    finally:
        eng.close()
    for k in base:
        assert again[k].tobytes() == base[k].tobytes(), k
    print(f"M {M} at {holders[:3]}, N {N} (largest window {m}): refused from {M * N} on")


# ---- a value at the limit of the micro-units ----
@pytest.mark.parametrize("cut", [False, True])
def test_a_planted_dp_of_2_38_micro_units_is_refused_naming_the_pair(cut, monkeypatch):
    """Valid haplotype frequencies give no finite D' near 274877.906944, so NGSLD_TEST_SCAN_PLANT_DP writes one into the record
    of one pair before the scan kernel reads it.  2^38 micro-units, of either sign, are refused naming the pair and leave no
    result; 2^38 - 1 are summed, and the windows are those of the table with that row's D' replaced; without the knob the
    context gives its earlier bytes."""
    raw, chrs, pos, where = _windowed()
    text, labels, _ = _windowed_table()
    ld, half = ("Dp", "r2"), 3000
    lines = text.splitlines(keepends=True)
    data = [k for k, ln in enumerate(lines) if ln.strip() and not ln.startswith("site1\t")]
    # record `at` of the plan is row `at` of the table: far from the first chunk, not a row's first candidate, and near enough
    # to lie inside a flank of some window
    at = next(k for k in range(2 * len(data) // 3, len(data))
              if (lambda g: labels.index(g[1]) > labels.index(g[0]) + 1 and 0 < int(g[2]) <= 1000)(lines[data[k]].split("\t")))
    f = lines[data[at]].split("\t")
    i, j = labels.index(f[0]), labels.index(f[1])
    assert j > i + 1 and all(math.isfinite(float(x)) for x in f[2:7])
    f[5] = "274877.906943"
    planted = "".join(lines[:data[at]] + ["\t".join(f)] + lines[data[at] + 1:])
    assert scan_ref.micro(f[5]) == 2 ** 38 - 1
    if cut:
        monkeypatch.setenv("NGSLD_TEST_SCAN_CHUNK_PAIRS", str(len(data) // 10))
        monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "7")
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True))
    try:
        base, st, _ = _check(eng, text, labels, where, half, ld=ld)
        assert (st["chunks"] > 1) == cut
        for value in ("274877.906944", "-274877.906944", "1e300"):
            monkeypatch.setenv("NGSLD_TEST_SCAN_PLANT_DP", f"{at}:{value}")
            with pytest.raises(capi.NgsldError) as e:
                eng.scan(half, ld=ld)
            assert e.value.code == capi.ERR_UNSUPPORTED, e.value.msg
            assert f"a scan value of the pair of sites {i} - {j} reaches 2^38 micro-units" in e.value.msg, e.value.msg
            assert eng._L.ngsld_scan_get(eng._h, 7, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
        win, _ = eng.scan(half, ld=("r2",))  # (D' is not chosen: the planted value is not read)
        assert win["sum_lr_r2"].tobytes() == base["sum_lr_r2"].tobytes()
        monkeypatch.setenv("NGSLD_TEST_SCAN_PLANT_DP", f"{at}:274877.906943")
        win, _, want = _check(eng, planted, labels, where, half, ld=ld)
        assert max(max(want[f"sum_{c}_Dp"]) for c in scan_ref.CLASSES) >= 2 ** 38 - 1
        assert win["sum_ll_Dp"].tobytes() != base["sum_ll_Dp"].tobytes() and win["sum_ll_r2"].tobytes() == base["sum_ll_r2"].tobytes()
        monkeypatch.delenv("NGSLD_TEST_SCAN_PLANT_DP")
        again, _ = eng.scan(half, ld=ld)
    finally:
        eng.close()
    for k in base:
        assert again[k].tobytes() == base[k].tobytes(), k


# ---- the other pair-kernel families ----
def _family_cases():
    from test_gpu_analyses_by_family import CASES
    return list(CASES)


@pytest.mark.parametrize("case", _family_cases())
def test_windowed_scan_under_every_kernel_family(case):
    """The 16- and 32-lane groups, run10, ab, multi, multi-ab with its _mono and _masked inputs and both streaming kernels, whose
    items are 5 or 20 candidates wide at pairs_per_item 5: no item is a whole wavefront."""
    import test_gpu_analyses_by_family as fam
    name, how, kernel, _, span = fam.CASES[case]
    inp = fam._input(name)
    where = list(zip(inp.chrs, (int(p) for p in inp.pos)))
    eng = fam._new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        short = kernel in ("multi", "multi-ab", "stream")  # (the families launched item by item: their items follow the tuning)
        if short:
            eng.set_tuning(pairs_per_item=5)
        fam._plan(eng, inp)
        if short:
            assert int(eng.items()["count"].max()) == 5 * span // 16 < 64
        text = fam._tsv(eng, inp)
        rows = scan_ref.counted_rows(text, inp.labels, ld=ALL4)
        for half in (500, 10000):
            _check(eng, text, inp.labels, where, half, rows=rows, ld=ALL4)
    finally:
        eng.close()
    assert fam.WIN["max_kb_dist"] == 20
    if name.endswith("_mono"):
        assert len(rows) < _n_rows(text)  # (non-finite rows drop out)


# ---- the binary ----
def test_cli_scan_out(tmp_path):
    n_sites, n_ind = 500, 64
    raw = synth.make_gl_numpy(n_sites, n_ind, 97, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 97, max_gap=300, n_chr=2)
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    g, p, ph = str(tmp_path / "g.bin"), str(tmp_path / "p.pos"), str(tmp_path / "ph.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    synth.write_pos(ph, chrs, pos, header=True, extra_col=True)
    common = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "20", "--extend_out"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, env=env: subprocess.run([*common, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300,  # noqa: E731
                                             env=env)
    sk = ["--scan_half_window", "5000", "--scan_ld", "Dp,r2", "--scan_min_maf", "0.05", "--scan_max_kb_dist", "15"]
    ref_kw = dict(ld=("Dp", "r2"), min_maf=0.05, max_kb_dist=15.0)
    # --scan_out alone: the file, no TSV (not even on standard output)
    r = run("--pos", p, "--scan_out", "s.tsv", *sk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> LD scan:" in r.stderr
    # beside --out: the table's bytes are those of a run without --scan_out
    r = run("--pos", p, "--out", "t.tsv", "--scan_out", "s2.tsv", *sk)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--pos", p, "--out", "t0.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    table = open(tmp_path / "t.tsv", "rb").read()
    assert table == open(tmp_path / "t0.tsv", "rb").read() and len(table) > 100_000
    want = scan_ref.scan_file(table.decode(), labels, 5000, **ref_kw)
    assert open(tmp_path / "s.tsv").read() == want
    assert open(tmp_path / "s2.tsv").read() == want
    assert "\tNA" in want and want.count("\n") == n_sites + 1
    # --posH and extra label columns: the site column is the label up to its first TAB
    r = run("--posH", ph, "--scan_out", "s3.tsv", *sk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "s3.tsv").read() == want
    # beside --site_out in one command
    r = run("--pos", p, "--scan_out", "s4.tsv", "--scan_half_window", "2000", "--site_out", "k.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "s4.tsv").read() == scan_ref.scan_file(table.decode(), labels, 2000)
    assert os.path.getsize(tmp_path / "k.tsv") > 0
    # without --pos the sites are numbered from 1 and every window is its own site
    nopos = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "0", "--max_snp_dist", "20"]
    r = subprocess.run([*nopos, "--out", "t5.tsv", "--scan_out", "s5.tsv", "--scan_half_window", "1000"], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = open(tmp_path / "s5.tsv").read()
    idx = [str(k + 1) for k in range(n_sites)]
    assert got == scan_ref.scan_file("", idx, 1000, names=idx, positions=scan_ref.NO_POS)
    assert got.splitlines()[1].split("\t")[:7] == ["1", "1", "1", "0", "0", "0", "0"]
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--pos", p, "--scan_out", "s6.tsv", *sk, env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--scan_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "s6.tsv")


# ---- "%f" ties: the scan of the reference program's own table ----
@pytest.mark.parametrize("name", ["called_n8", "called_n16"])
def test_scan_of_the_reference_table_at_ties(name, tmp_path):
    import test_gpu_ties as ties
    if not ties.have_ref_program():
        pytest.skip("oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")
    case = ties.Case(name, str(tmp_path))
    assert int(case.d_ties.sum()) >= case.min_d
    text = ties._ref_table(case, True, str(tmp_path))
    where = list(zip(case.chrs, (int(p) for p in case.pos)))
    eng = case.engine()
    try:
        eng.plan(extend_out=True)
        rows = scan_ref.counted_rows(text, case.labels, ld=ALL4)
        win, stats = eng.scan(2000, ld=ALL4)
        _same(win, scan_ref.scan(text, case.labels, 2000, positions=where, rows=rows, ld=ALL4), ALL4)
        assert stats["pairs"] == len(case.rec) and stats["pairs_counted"] == len(rows) > 0
        win, _ = eng.scan(10 ** 9, ld=("D",))
        _same(win, scan_ref.scan(text, case.labels, 10 ** 9, positions=where, ld=("D",)), ("D",))
    finally:
        eng.close()
