"""LD across chromosomes on the device (ngsld_cross_ld, Engine.cross_ld, the binary's --cross_* flags) against
tests/cross_ref.py -- the rule of CROSS.md in plain Python -- applied to the same engine's own TSV (run_text).  Every cell key, n,
sum, max and linked must be equal as integers and every mean bit for bit: nothing sampled, no tolerance.

The input is all pairs of 300 sites (44,850 rows) over four chromosomes of unequal size, one of a single site: the rows of a site
start at every offset of an item, so the chromosome borders fall at every lane.

GPU time of this file on one MI355X: see CROSS.md ("What the tests cost")."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cross_ref
import site_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
SIZES = (("chrA", 97), ("chrB", 1), ("chrC", 140), ("chrD", 62))
N_SITES = sum(n for _, n in SIZES)
N_PAIRS = N_SITES * (N_SITES - 1) // 2
KNOBS = ("CROSS_CHUNK_PAIRS", "CROSS_SPAN_ITEMS", "CROSS_PLANT_DP", "RECORD_SLICE_ITEMS", "SUM_WRAP_LIMIT", "GRID_LDS_BYTES",
         "GRID_CHUNK_PAIRS")
U, I = capi.ERR_UNSUPPORTED, capi.ERR_INVALID


def _positions(sizes=SIZES):
    chrs, pos = [], []
    for k, (name, n) in enumerate(sizes):
        _, p = synth.make_positions(n, 61 + k, max_gap=300)
        chrs += [name] * n
        pos += [int(x) for x in p]
    return chrs, np.array(pos, dtype=np.int64)


CHRS, POS = _positions()
LABELS = [f"{c}:{int(p)}" for c, p in zip(CHRS, POS)]
ALL = dict(extend_out=True)  # (all pairs: max_kb_dist 0; extend_out: the restatement applies the maf filter where the TSV has maf1 / maf2)
# name: (n_ind, synth kw, plan kw, geno kw)
INPUTS = {
    "n8": (8, {}, ALL, None),
    "n64": (64, {}, ALL, None),
    "n500": (500, {}, ALL, None),
    # (the sites' frequencies lie between 0.15 and 0.36: both maf filters, the plan's and the call's, drop some)
    "rnd64": (64, {}, dict(min_maf=0.26, rnd_sample=0.6, seed=7, extend_out=True), None),
    "mono64": (64, dict(mono_frac=0.2), ALL, None),
    "call64": (64, {}, ALL, dict(call_geno=(0.1, 0.9))),
}
_made = {}


def _new_engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _tsv(eng, labels):
    eng.set_text_output(labels)
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for eng, _ in _made.values():
        eng.close()
    _made.clear()


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv("NGSLD_TEST_" + k, raising=False)


def _input(name):
    """(engine, its TSV): made once.  The table first: ngsld_set_text_output makes the stores of the plan stale."""
    if name not in _made:
        n_ind, skw, plan_kw, geno_kw = INPUTS[name]
        raw = synth.make_gl_numpy(N_SITES, n_ind, 700 + n_ind, depth=4.0, **skw)
        eng = _new_engine(raw, CHRS, POS, plan_kw, geno_kw)
        _made[name] = (eng, _tsv(eng, LABELS))
    return _made[name]


_wanted = {}


def _want(name, text, labels, bin_size, **kw):
    """cross_ref.cross, once per input and setting: a restatement over 44,850 rows takes a moment."""
    key = (name, bin_size, tuple(sorted(kw.items())))
    if key not in _wanted:
        _wanted[key] = cross_ref.cross(text, labels, bin_size, **kw)
    return _wanted[key]


def _same(cells, want, ld):
    chosen = [f for f in site_ref.FIELDS if f in ld]
    assert set(cells) == {"chr1", "bin1", "chr2", "bin2", "n"} | {f"{w}_{f}" for f in chosen for w in ("sum", "max", "linked", "mean")}
    for k in ("chr1", "chr2"):
        assert [str(x) for x in cells[k]] == want[k], k
    for k in ("bin1", "bin2", "n"):
        assert [int(x) for x in cells[k]] == want[k], k
    for f in chosen:
        for w in ("sum", "max", "linked"):
            assert [int(x) for x in cells[f"{w}_{f}"]] == want[f"{w}_{f}"], (w, f)
        exp = np.array(want[f"mean_{f}"], dtype=np.float64)
        got = cells[f"mean_{f}"]
        bad = np.nonzero(got.view(np.int64) != exp.view(np.int64))[0]
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _bytes(cells):
    return {k: (v.tobytes() if v.dtype.kind != "U" else tuple(v)) for k, v in cells.items()}


def _check(name, bin_size=0, **kw):
    eng, text = _input(name)
    cells, stats = eng.cross_ld(LABELS, bin_size, **kw)
    want = _want(name, text, LABELS, bin_size, **kw)
    _same(cells, want, kw.get("ld", ("r2",)))
    rows = sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))
    assert stats["pairs"] == rows
    assert stats["pairs_counted"] == sum(want["n"]) and stats["cells"] == len(want["n"])
    assert stats["pairs_cross"] == sum(n for n, a, b in zip(want["n"], want["chr1"], want["chr2"]) if a != b)
    assert stats["lds"] == 0 and stats["span_items"] >= 1
    print(f"{name} B {bin_size} pairs {stats['pairs']} counted {stats['pairs_counted']} across {stats['pairs_cross']} cells "
          f"{stats['cells']} bins {stats['bins']} span {stats['span_items']} chunks {stats['chunks']} pairs_ms {stats['pairs_ms']:.2f} "
          f"cross_ms {stats['cross_ms']:.3f} total_ms {stats['total_ms']:.2f}")
    return cells, stats, want


# ---- 1. the rule on the engine's own table ----
CASES = {
    # name: (input, bin_size, cross kw)
    "n8_chromosomes": ("n8", 0, {}),
    "n8_windows": ("n8", 2000, {}),
    "n64_chromosomes": ("n64", 0, {}),
    "n500_chromosomes": ("n500", 0, {}),
    "n500_windows": ("n500", 2000, {}),
    "all_four": ("n64", 2000, dict(ld=ALL4, linked_min=0.2)),
    "signed_D_Dp": ("n64", 2000, dict(ld=("D", "Dp"), abs_value=False, linked_min=0.1)),
    "min_maf_rnd_sample": ("rnd64", 2000, dict(min_maf=0.3)),
    "uncalled_mono": ("mono64", 2000, dict(ld=ALL4)),
    "call_geno": ("call64", 2000, dict(ld=("r2", "Dp"))),
    "only_across": ("n64", 2000, dict(within=False, ld=("r2", "D"))),
    "min_kb_dist_inside_a_chromosome": ("n64", 2000, dict(min_kb_dist=5.0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cross_ld_equals_the_rule_on_own_tsv(case):
    name, bin_size, kw = CASES[case]
    cells, stats, want = _check(name, bin_size, **kw)
    assert stats["pairs_cross"] > 0 and set(want["chr1"]) | set(want["chr2"]) >= {"chrA", "chrC", "chrD"}
    assert ("chrB", "chrB") not in set(zip(want["chr1"], want["chr2"]))  # (a chromosome of one site has no pair of its own)
    if bin_size == 0:
        assert stats["bins"] == 4 and stats["cells"] == 9  # (every pair of chromosomes but chrB with itself)
    if case == "uncalled_mono":
        assert stats["pairs_counted"] < stats["pairs"]  # (NaN rows)
    if case == "min_maf_rnd_sample":
        assert stats["pairs"] < N_PAIRS and stats["pairs_counted"] < stats["pairs"]
    if case == "signed_D_Dp":
        _, text = _input(name)
        assert want["sum_D"] != _want(name, text, LABELS, bin_size, **{**kw, "abs_value": True})["sum_D"]
    if case == "only_across":
        assert stats["pairs_counted"] == stats["pairs_cross"] and all(a != b for a, b in zip(want["chr1"], want["chr2"]))
    if case == "min_kb_dist_inside_a_chromosome":
        whole = _check(name, bin_size)[1]
        assert stats["pairs_cross"] == whole["pairs_cross"] and 0 < stats["pairs_counted"] - stats["pairs_cross"] < \
            whole["pairs_counted"] - whole["pairs_cross"]


@pytest.mark.parametrize("bin_size", [0, 2000, 137, 10 ** 9])
def test_bin_sizes_on_one_input(bin_size):
    """137: some 330 bins, 55,000 cells, a run changes every few lanes; 10^9: every site in bin 0 of its chromosome -- B = 0's
    cells.  Whatever the bins, every counted row is in one cell."""
    kw = dict(ld=ALL4, abs_value=False, linked_min=0.3)
    cells, stats, want = _check("n64", bin_size, **kw)
    per_chr, st0, _ = _check("n64", 0, **kw)
    assert stats["pairs"] == N_PAIRS and stats["pairs_counted"] == st0["pairs_counted"] > 0 and stats["pairs_cross"] == st0["pairs_cross"]
    for f in ALL4:
        assert int(cells[f"sum_{f}"].sum()) == int(per_chr[f"sum_{f}"].sum()), f
        assert int(cells[f"linked_{f}"].sum()) == int(per_chr[f"linked_{f}"].sum()), f
    if bin_size == 10 ** 9:
        assert _bytes(cells) == _bytes(per_chr)
    if bin_size == 137:
        assert stats["bins"] > 300 and stats["cells"] > 20000
    # without labels at B = 0: the same cells under the chromosomes' ordinals
    if bin_size == 0:
        eng, _ = _input("n64")
        by_ordinal, _ = eng.cross_ld(None, 0, **kw)
        names = {c: str(k + 1) for k, (c, _) in enumerate(SIZES)}
        assert [names[c] for c in cells["chr1"]] == list(by_ordinal["chr1"]) and [names[c] for c in cells["chr2"]] == list(by_ordinal["chr2"])
        assert all(by_ordinal[k].tobytes() == cells[k].tobytes() for k in cells if not k.startswith("chr"))


# ---- 2. against what exists ----
@pytest.mark.parametrize("bin_size", [2000, 137])
def test_same_chromosome_cells_are_the_grids_and_the_parts_add_up(bin_size):
    eng, _ = _input("n64")
    kw = dict(ld=ALL4, abs_value=False, linked_min=0.3)
    whole, sw = eng.cross_ld(LABELS, bin_size, **kw)
    across, sa = eng.cross_ld(LABELS, bin_size, within=False, **kw)
    grid, sg = eng.grid(LABELS, bin_size, **kw)
    same = whole["chr1"] == whole["chr2"]
    assert 0 < int(same.sum()) < len(same)
    assert list(whole["chr1"][same]) == list(grid["chr"])
    for k in grid:
        if k != "chr":
            assert whole[k][same].tobytes() == grid[k].tobytes(), k
    # the rows across two chromosomes and the rows inside one partition the whole
    assert list(whole["chr1"][~same]) == list(across["chr1"]) and list(whole["chr2"][~same]) == list(across["chr2"])
    for k in across:
        if not k.startswith("chr"):
            assert whole[k][~same].tobytes() == across[k].tobytes(), k
    assert int(whole["n"].sum()) == sw["pairs_counted"] and int(whole["n"][~same].sum()) == sw["pairs_cross"] == sa["pairs_counted"]
    assert sw["pairs_counted"] - sw["pairs_cross"] == sg["pairs_counted"]


# ---- 3. every span, chunk and slice: the same bytes ----
def test_spans_chunks_and_slices_give_the_same_bytes(monkeypatch):
    """Several chromosomes, windows of 2,000 bp: a wavefront's span crosses row ends, chromosome borders and chunk ends."""
    kw = dict(ld=ALL4, abs_value=False, linked_min=0.3)
    base, s0, _ = _check("n64", 2000, **kw)
    eng, _ = _input("n64")
    assert s0["chunks"] == 1
    for env in ({"CROSS_SPAN_ITEMS": "1"}, {"CROSS_SPAN_ITEMS": "3"}, {"CROSS_SPAN_ITEMS": "1000000"},
                {"CROSS_CHUNK_PAIRS": "3000"}, {"CROSS_CHUNK_PAIRS": "3000", "CROSS_SPAN_ITEMS": "5", "RECORD_SLICE_ITEMS": "7"},
                {"RECORD_SLICE_ITEMS": "7", "CROSS_SPAN_ITEMS": "3"}):
        for k in KNOBS:
            monkeypatch.delenv("NGSLD_TEST_" + k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv("NGSLD_TEST_" + k, v)
        cells, st = eng.cross_ld(LABELS, 2000, **kw)
        assert _bytes(cells) == _bytes(base), env
        assert st["span_items"] == min(int(env.get("CROSS_SPAN_ITEMS", s0["span_items"])), 1 << 20)
        assert (st["chunks"] > 5) == ("CROSS_CHUNK_PAIRS" in env)


def test_a_carried_cell_passes_255_and_65535_rows(monkeypatch):
    """One chromosome of 720 sites at B = 0: 258,840 rows in one cell.  A span of three items carries 192 rows, the default span
    passes 255, a span of the whole launch carries every row of the chunk through one wavefront's registers: a count packed
    into a byte, or into sixteen bits, wraps."""
    n = 720
    chrs, pos = synth.make_positions(n, 83, max_gap=300)
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    raw = synth.make_gl_numpy(n, 8, 783, depth=4.0)
    eng = _new_engine(raw, chrs, pos, dict(extend_out=True))
    try:
        text = _tsv(eng, labels)
        want = cross_ref.cross(text, labels, 0, ld=ALL4, linked_min=0.0)
        assert len(want["n"]) == 1 and n * (n - 1) // 2 >= want["n"][0] == want["linked_r2"][0] > 3 * 65535
        out = []
        for env in ({}, {"CROSS_SPAN_ITEMS": "1"}, {"CROSS_SPAN_ITEMS": "3"}, {"CROSS_SPAN_ITEMS": "1000000"},
                    {"CROSS_CHUNK_PAIRS": "3000"}, {"RECORD_SLICE_ITEMS": "7"}, {"CROSS_CHUNK_PAIRS": "3000", "RECORD_SLICE_ITEMS": "7"}):
            for k in KNOBS:
                monkeypatch.delenv("NGSLD_TEST_" + k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv("NGSLD_TEST_" + k, v)
            a, sa = eng.cross_ld(labels, 0, ld=ALL4, linked_min=0.0)
            b, sb = eng.cross_ld(labels, 0, ld=ALL4, linked_min=0.0)  # (two calls in a row: the same bytes)
            assert _bytes(a) == _bytes(b) and sa["chunks"] == sb["chunks"]
            _same(a, want, ALL4)
            if not env:
                assert sa["span_items"] * 64 > 255
            out.append(a)
        assert all(_bytes(a) == _bytes(out[0]) for a in out)
    finally:
        eng.close()


# ---- 4. the guard of the sums, a value beyond 2^38 micro-units ----
def _getters_refuse(eng):
    got = C.c_uint64(0)
    assert eng._L.ngsld_cross_ld_cells(eng._h, 0, None, None, None, None, None, C.byref(got)) == I
    assert b"no ngsld_cross_ld result" in eng._L.ngsld_last_error(eng._h)
    assert eng._L.ngsld_cross_ld_chromosomes(eng._h, 0, None, None) == I
    assert eng._L.ngsld_cross_ld_get(eng._h, 7, 0, None, None, None, None) == I


def test_the_sum_guard_is_pinned_to_the_unit(monkeypatch):
    """NGSLD_TEST_SUM_WRAP_LIMIT = L: refused from max |q| x (the rows a cell can hold) >= L on.  M from the table, the row bound
    from the bins (the product of the two largest bin populations, or the pairs inside the largest): L = M x N is refused,
    M x N + 1 accepted."""
    eng, text = _input("n64")
    kw = dict(ld=("D", "Dp"), abs_value=False)
    base, _, want = _check("n64", 2000, **kw)
    M = 0
    for ln in text.splitlines():
        f = ln.split("\t")
        if not ln or f[0] == "site1":
            continue
        qs = [site_ref.micro(f[4]), site_ref.micro(f[5])]
        if None not in qs:
            M = max(M, max(abs(q) for q in qs))
    pop = sorted(np.bincount([g for g, _, _ in (cross_ref.gbins(LABELS, 2000)[lab] for lab in LABELS)]), reverse=True)
    N = min(max(int(pop[0]) * int(pop[1]), int(pop[0]) * (int(pop[0]) - 1) // 2), N_PAIRS)
    assert M > 0 and N >= max(want["n"])
    monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(M * N))
    with pytest.raises(capi.NgsldError) as e:
        eng.cross_ld(LABELS, 2000, **kw)
    assert e.value.code == U and e.value.msg.startswith("LD across chromosomes:") and "too large to sum exactly" in e.value.msg
    assert f"up to {N} pairs" in e.value.msg
    _getters_refuse(eng)
    for limit in (M * N + 1, 2 ** 63):  # (one unit more; tracking on at the shipped limit)
        monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(limit))
        assert _bytes(eng.cross_ld(LABELS, 2000, **kw)[0]) == _bytes(base)


def test_a_planted_value_on_either_side_of_2_38_micro_units(monkeypatch):
    """No input gives a finite D' near 2^38 micro-units: NGSLD_TEST_CROSS_PLANT_DP puts one into a record.  274877.906943 is the
    largest value allowed and is summed; 274877.906944 is refused, naming the pair, the store is empty and the context usable."""
    eng, text = _input("n64")
    rows = [ln.split("\t") for ln in text.splitlines() if ln and not ln.startswith("site1\t")]  # (record k of the plan is row k)
    at = next(k for k in range(30000, len(rows)) if rows[k][0].startswith("chrC") and rows[k][1].startswith("chrD")
              and (site_ref.micro(rows[k][5]) or 0) >= 500000)  # (linked before and after)
    s1, s2 = LABELS.index(rows[at][0]), LABELS.index(rows[at][1])
    kw = dict(ld=("Dp",), abs_value=False)
    base, _, _ = _check("n64", 0, **kw)
    cell = next(k for k in range(len(base["n"])) if (base["chr1"][k], base["chr2"][k]) == ("chrC", "chrD"))
    monkeypatch.setenv("NGSLD_TEST_CROSS_CHUNK_PAIRS", "3000")  # (the record lies in a later chunk)
    monkeypatch.setenv("NGSLD_TEST_CROSS_PLANT_DP", f"{at}:274877.906943")
    cells, _ = eng.cross_ld(LABELS, 0, **kw)
    assert int(cells["max_Dp"][cell]) == 2 ** 38 - 1
    assert int(cells["sum_Dp"][cell]) == int(base["sum_Dp"][cell]) - site_ref.micro(rows[at][5]) + 2 ** 38 - 1
    assert all(cells[k].tobytes() == base[k].tobytes() for k in ("n", "linked_Dp"))
    monkeypatch.setenv("NGSLD_TEST_CROSS_PLANT_DP", f"{at}:-274877.906944")
    with pytest.raises(capi.NgsldError) as e:
        eng.cross_ld(LABELS, 0, **kw)
    assert e.value.code == U and f"the pair of sites {s1} - {s2}" in e.value.msg and "2^38" in e.value.msg
    assert "LD across chromosomes" in e.value.msg
    _getters_refuse(eng)
    monkeypatch.delenv("NGSLD_TEST_CROSS_PLANT_DP")
    assert _bytes(eng.cross_ld(LABELS, 0, **kw)[0]) == _bytes(base)


# ---- 5. refusals, the store ----
def _refused(eng, labels, bin_size, code, *words, **kw):
    with pytest.raises(capi.NgsldError) as e:
        eng.cross_ld(labels, bin_size, **kw)
    assert e.value.code == code and all(w in e.value.msg for w in words), (e.value.code, e.value.msg)
    if code == U:
        assert e.value.msg.startswith("LD across chromosomes:"), e.value.msg
    _getters_refuse(eng)


def test_refusals():
    eng, _ = _input("n8")
    assert eng.cross_ld(LABELS, 2000)[1]["cells"] > 0
    a0, b0, c0 = 0, 97, 98  # (the first sites of chrA, chrB, chrC)
    # positions: not digits, decreasing -- read only where a bin_size asks for them
    for bad in ("chrA:12a", "chrA:", "chrA", "chrA:-5", "chrA:1e3", "chrA:" + "9" * 20):
        _refused(eng, LABELS[:7] + [bad] + LABELS[8:], 2000, U, f'"{bad}"', "not plain decimal digits")
    assert eng.cross_ld(LABELS[:7] + ["chrA:x"] + LABELS[8:], 0)[1]["cells"] == 9
    swapped = LABELS[:10] + [LABELS[11], LABELS[10]] + LABELS[12:]
    _refused(eng, swapped, 2000, U, f'"{LABELS[10]}"', f'"{LABELS[11]}"', "below that of the site before it")
    # chromosomes: labels against pos_dist, both ways; a name that begins two runs -- at either bin_size
    for B in (0, 2000):
        again = LABELS[:c0] + [f"chrB:{int(p)}" for p in POS[c0:c0 + 140]] + LABELS[c0 + 140:]
        _refused(eng, again, B, U, f'"{again[c0]}"', "but their distance is not finite")
        early = LABELS[:50] + [f"chrE:{int(p)}" for p in POS[50:b0]] + LABELS[b0:]
        _refused(eng, early, B, U, f'"{early[50]}"', f'"{early[49]}"', "but their distance is finite")
        aba = [f"{'chrA' if c == 'chrC' else c}:{int(p)}" for c, p in zip(CHRS, POS)]
        _refused(eng, aba, B, U, 'chromosome "chrA" begins a second time', f'"{aba[c0]}"')
    # labels, parameters
    _refused(eng, None, 2000, I, "labels are NULL")
    _refused(eng, ["(null)"] * N_SITES, 2000, I, "(null)")
    for b in (2 ** 31, 2 ** 40):
        _refused(eng, LABELS, b, I, "bin_size")
    _refused(eng, LABELS, 2000, I, "linked_min is NaN", linked_min=math.nan)
    _refused(eng, LABELS, 2000, I, "min_maf is NaN", min_maf=math.nan)
    for bad in (math.nan, -1.0, math.inf):
        _refused(eng, LABELS, 2000, I, "min_kb_dist", min_kb_dist=bad)
    # the accumulators: windows of one base are tens of thousands of bins, half their square in cells
    _refused(eng, LABELS, 1, U, "bins", "cells", "2 GiB", "a larger bin_size is needed")
    assert eng.cross_ld(LABELS, 2000)[1]["cells"] > 0  # (a refusal leaves the context usable)
    arr = (C.c_char_p * N_SITES)(*[l.encode() for l in LABELS])
    p = capi.CrossLdParams(C.sizeof(capi.CrossLdParams) - 8, 8, 2000, 0.0, 0.5, 0.0, 1, 1)
    assert eng._L.ngsld_cross_ld(eng._h, C.byref(p), arr, None) == I and b"struct_size" in eng._L.ngsld_last_error(eng._h)
    _getters_refuse(eng)
    p = capi.CrossLdParams(C.sizeof(capi.CrossLdParams), 8, 2000, 0.0, 0.5, 0.0, 1, 1)
    st = capi.CrossLdStats()  # (struct_size not set)
    assert eng._L.ngsld_cross_ld(eng._h, C.byref(p), arr, C.byref(st)) == I
    for fields in (0, 16):  # (an empty statistic set, an unknown one)
        p.fields = fields
        assert eng._L.ngsld_cross_ld(eng._h, C.byref(p), arr, None) == I and b"fields" in eng._L.ngsld_last_error(eng._h)
    p.fields = 8
    assert eng._L.ngsld_cross_ld(eng._h, C.byref(p), arr, None) == capi.OK  # (stats may be NULL)


def test_refusals_of_the_position_gaps():
    raw = synth.make_gl_numpy(120, 8, 5, depth=4.0)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.plan(extend_out=True)  # (no ngsld_set_pos_dist: every gap is +inf)
        labels = [f"c:{10 * k + 10}" for k in range(120)]
        _refused(eng, labels, 0, I, "no position gaps")
        _refused(eng, None, 0, I, "no position gaps")
        eng.set_pos_dist(np.full(120, 10.5))  # (positions no file holds: half a base between sites)
        eng.plan(extend_out=True)
        _refused(eng, labels, 100, U, "min_kb_dist", "integer position gaps", min_kb_dist=0.5)
        assert eng.cross_ld(labels, 100)[1]["pairs_counted"] > 0  # (no floor: only whether dist is finite matters)
    finally:
        eng.close()


def test_the_result_goes_with_the_plan():
    raw = synth.make_gl_numpy(N_SITES, 16, 91, depth=4.0)
    eng = _new_engine(raw, CHRS, POS, ALL)
    try:
        cells, st = eng.cross_ld(LABELS, 2000, ld=("r2", "Dp"))
        n = np.zeros(max(int(st["cells"]), 1), dtype=np.uint64)
        got = C.c_uint64(0)
        assert eng._L.ngsld_cross_ld_cells(eng._h, len(n), None, None, None, None, n.ctypes.data, C.byref(got)) == capi.OK
        assert got.value == st["cells"] > 0 and n.tobytes() == cells["n"].tobytes()
        assert eng._L.ngsld_cross_ld_get(eng._h, 5, len(n), None, None, None, None) == I  # (D was not chosen)
        assert eng._L.ngsld_cross_ld_get(eng._h, 6, len(n), None, None, None, None) == capi.OK
        grid, _ = eng.grid(LABELS, 2000)  # (another analysis leaves this store alone)
        assert eng._L.ngsld_cross_ld_cells(eng._h, 0, None, None, None, None, None, C.byref(got)) == capi.OK and got.value == st["cells"]
        eng.plan(**ALL)
        _getters_refuse(eng)
        eng.cross_ld(LABELS, 0)
        eng.set_pos_dist(shard.pos_dist_from_positions(CHRS, POS))
        _getters_refuse(eng)
    finally:
        eng.close()


# ---- 6. the binary ----
def test_cli_cross_out(tmp_path):
    n_ind = 64
    raw = synth.make_gl_numpy(N_SITES, n_ind, 97, depth=4.0, mono_frac=0.1)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, CHRS, POS)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(N_SITES), "--pos", p, "--max_kb_dist", "0", "--extend_out"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, env=env: subprocess.run([*base, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300,  # noqa: E731
                                             env=env)
    ck = ["--cross_bin_size", "2000", "--cross_ld", "Dp,r2", "--cross_min_maf", "0.05", "--cross_linked_min", "0.3", "--cross_min_kb_dist", "3"]
    ref_kw = dict(ld=("Dp", "r2"), min_maf=0.05, linked_min=0.3, min_kb_dist=3.0)
    # --cross_out alone: the file, no TSV (not even on standard output)
    r = run("--cross_out", "s.tsv", *ck)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> LD across chromosomes: " in r.stderr and " across chromosomes\n" in r.stderr
    # with the table beside it: the table's bytes are those of a run without --cross_out
    r = run("--out", "t.tsv", "--cross_out", "s2.tsv", *ck)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--out", "t0.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    table = open(tmp_path / "t.tsv", "rb").read()
    assert table == open(tmp_path / "t0.tsv", "rb").read() and len(table) > 100_000
    want = cross_ref.cross_file(table.decode(), LABELS, 2000, **ref_kw)
    assert len(want.splitlines()) > 100 and "chrA\t0\tchrD\t" in want
    assert open(tmp_path / "s.tsv").read() == want
    assert open(tmp_path / "s2.tsv").read() == want
    # per chromosome, signed, only across; beside another analysis
    r = run("--cross_out", "s3.tsv", "--cross_ld", "D", "--cross_signed", "--cross_only", "--grid_out", "g.tsv", "--grid_bin_size", "2000")
    assert r.returncode == 0, r.stderr[-2000:]
    want = cross_ref.cross_file(table.decode(), LABELS, 0, ld=("D",), abs_value=False, within=False)
    assert open(tmp_path / "s3.tsv").read() == want and 4 <= len(want.splitlines()) <= 7
    assert os.path.getsize(tmp_path / "g.tsv") > 0
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--cross_out", "s5.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--cross_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "s5.tsv")


# ---- 7. printed ties: the reference program's table ----
def test_printed_ties_are_held_to_the_reference_programs_table(tmp_path, monkeypatch):
    """300 sites of 8 called individuals, all pairs, D: some 1,500 values are exact "%f" ties (odd / 128 and the like).  The cells
    are held to the rule on the REFERENCE program's table, built the way tests/test_gpu_ties.py builds its own -- the engine's
    own table would bend with a wrong device value --, with linked_min on the value the commonest tie prints and on both of its
    neighbours, in one chunk and in sixteen."""
    from oracle import orc
    from printed_values import is_tie, micro
    from util import have_ref_program, run_ref_program
    if not have_ref_program():
        pytest.skip("oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")
    n_ind = 8
    raw = np.eye(3)[synth.make_gl_numpy(N_SITES, n_ind, 7 + n_ind, depth=8.0).argmax(2)]
    pd = shard.pos_dist_from_positions(CHRS, POS)
    ppath, gpath, out = (str(tmp_path / f) for f in ("in.pos", "in.glf", "ref.tsv"))
    synth.write_pos(ppath, CHRS, POS)
    raw.tofile(gpath)
    rec = orc.Oracle(raw, pd, n_threads=8).run()
    ties = is_tie(rec["D"])
    assert int(ties.sum()) >= 1000
    flags = ["--n_ind", str(n_ind), "--n_sites", str(N_SITES), "--verbose", "0", "--pos", ppath, "--geno", gpath, "--max_kb_dist", "0",
             "--extend_out"]
    r = run_ref_program(rec, N_SITES, flags, out, str(tmp_path), threads=4)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    vals, counts = np.unique(np.abs(rec["D"][ties]), return_counts=True)
    q = micro(float(vals[np.argmax(counts)]))
    eng = _new_engine(raw, CHRS, POS, ALL)
    try:
        linked = []
        for floor in (q, q + 1, q - 1):
            kw = dict(ld=("D", "r2"), linked_min=floor / 10 ** 6)
            want = cross_ref.cross(text, LABELS, 2000, **kw)
            both = []
            for chunk in (None, "3000"):
                monkeypatch.delenv("NGSLD_TEST_CROSS_CHUNK_PAIRS", raising=False)
                if chunk:
                    monkeypatch.setenv("NGSLD_TEST_CROSS_CHUNK_PAIRS", chunk)
                cells, st = eng.cross_ld(LABELS, 2000, **kw)
                _same(cells, want, kw["ld"])
                assert (st["chunks"] > 5) == bool(chunk) and st["pairs_cross"] > 0
                both.append(cells)
            assert _bytes(both[0]) == _bytes(both[1])
            linked.append(sum(want["linked_D"]))
        # the table has rows exactly on the threshold: linked at q, not at q + 1
        assert linked[0] > linked[1] and linked[2] >= linked[0]
    finally:
        eng.close()
