"""The LD grid on the device (ngsld_grid, Engine.grid, the binary's --grid_* flags) against tests/grid_ref.py -- the rule of
GRID.md in plain Python -- applied to the same engine's own TSV (run_text).  Every cell key, n, sum, max and linked must be equal
as integers and every mean bit for bit: nothing sampled, no tolerance.

GPU time of this file on one MI355X: see GRID.md ("What the tests cost")."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import grid_ref
import site_ref
from ngsld_amd import capi, shard, synth
from printed_values import is_tie, micro

pytestmark = pytest.mark.gpu

KNOBS = ("NGSLD_TEST_GRID_LDS_BYTES", "NGSLD_TEST_GRID_CHUNK_PAIRS")


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _labels(chrs, pos):
    return [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]


def _tsv(eng, labels):
    eng.set_text_output(labels)
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _same(cells, want, ld):
    chosen = [f for f in site_ref.FIELDS if f in ld]
    assert set(cells) == {"chr", "bin1", "bin2", "n"} | {f"{w}_{f}" for f in chosen for w in ("sum", "max", "linked", "mean")}
    assert [str(x) for x in cells["chr"]] == want["chr"]
    for k in ("bin1", "bin2", "n"):
        assert [int(x) for x in cells[k]] == want[k], k
    for f in chosen:
        for w in ("sum", "max", "linked"):
            assert [int(x) for x in cells[f"{w}_{f}"]] == want[f"{w}_{f}"], (w, f)
        exp = np.array(want[f"mean_{f}"], dtype=np.float64)
        got = cells[f"mean_{f}"]
        bad = np.nonzero(got.view(np.int64) != exp.view(np.int64))[0]
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _check(eng, text, labels, bin_size, **kw):
    cells, stats = eng.grid(labels, bin_size, **kw)
    want = grid_ref.grid(text, labels, bin_size, **kw)
    _same(cells, want, kw.get("ld", ("r2",)))
    assert stats["pairs"] == sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))
    assert stats["pairs_counted"] == sum(want["n"]) and stats["cells"] == len(want["n"])
    print(f"B {bin_size} pairs {stats['pairs']} counted {stats['pairs_counted']} cells {stats['cells']} bins {stats['bins']} band "
          f"{stats['band']} lds {stats['lds']} chunks {stats['chunks']} pairs_ms {stats['pairs_ms']:.2f} grid_ms {stats['grid_ms']:.3f} "
          f"total_ms {stats['total_ms']:.2f}")
    return cells, stats, want


def _case(raw, chrs, pos, plan_kw, bin_size, grid_kw, geno_kw=None, labels=None):
    labels = labels or _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, labels)
        cells, stats, want = _check(eng, text, labels, bin_size, **grid_kw)
    finally:
        eng.close()
    return cells, stats, want, text


# extend_out everywhere: the restatement applies the maf filter where the TSV has maf1 / maf2
WIN = dict(max_kb_dist=20, extend_out=True)
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, grid kw, geno kw)
    "n8_window": (500, 8, {}, 1, WIN, {}, None),
    "n64_window": (500, 64, {}, 1, WIN, {}, None),
    "n500_window": (400, 500, {}, 1, WIN, {}, None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=20, min_maf=0.1, rnd_sample=0.6, seed=7, extend_out=True), dict(min_maf=0.15), None),
    "all_four": (400, 64, {}, 1, WIN, dict(ld=ALL4, linked_min=0.2), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, dict(ld=ALL4), None),
    "call_geno": (500, 64, {}, 1, WIN, dict(ld=("r2", "Dp")), dict(call_geno=(0.1, 0.9))),
    "max_snp_dist": (500, 64, {}, 2, dict(max_snp_dist=40, extend_out=True), dict(ld=("Dp", "r2")), None),
    "signed_D_Dp": (400, 64, {}, 1, WIN, dict(ld=("D", "Dp"), abs_value=False, linked_min=0.1), None),
    "kb_limit_inside_the_window": (400, 64, {}, 1, WIN, dict(max_kb_dist=7.5, ld=("D", "r2")), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_grid_equals_the_rule_on_own_tsv(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n_sites, n_ind, skw, n_chr, plan_kw, grid_kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 500 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 37, max_gap=300, n_chr=n_chr)
    _, stats, want, text = _case(raw, chrs, pos, plan_kw, 2000, grid_kw, geno_kw)
    assert stats["pairs_counted"] > 0 and stats["lds"] == 1
    assert len(set(want["chr"])) == n_chr and any(a != b for a, b in zip(want["bin1"], want["bin2"]))
    if name == "uncalled_mono":
        assert stats["pairs_counted"] < stats["pairs"]  # (NaN rows)
    if name == "signed_D_Dp":
        # (the table holds negative D: the signed sums are not the absolute ones)
        assert want["sum_D"] != grid_ref.grid(text, _labels(chrs, pos), 2000, **{**grid_kw, "abs_value": True})["sum_D"]


@functools.lru_cache(maxsize=1)
def _one_input():
    """600 sites over two chromosomes, un-called, a 30 kb window: the input of the bin sizes and of the launch shapes."""
    raw = synth.make_gl_numpy(600, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(600, 71, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True))
    try:
        text = _tsv(eng, labels)
        sites, sst = eng.site_ld(ld=ALL4, abs_value=False, linked_min=0.3)
    finally:
        eng.close()
    return raw, chrs, pos, labels, text, sites, sst


@pytest.mark.parametrize("bin_size", [137, 2000, 10 ** 9])
def test_bin_sizes_on_one_input_add_up_to_site_ld(bin_size, monkeypatch):
    """137: a band of some 220 bins, the rows of a tile span some twenty row bins and the window is far beyond what pays in LDS
    (the global path; forced into LDS at 64 KiB it still does not fit); 10^9: one cell per chromosome.  Whatever the
    bins, every counted row is in one cell: the cells' rows are ngsld_site_ld's counted rows, their sums half its per-site sums."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels, text, sites, sst = _one_input()
    kw = dict(ld=ALL4, abs_value=False, linked_min=0.3)
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True))
    try:
        cells, stats, want = _check(eng, text, labels, bin_size, **kw)
    finally:
        eng.close()
    assert int(cells["n"].sum()) == sst["pairs_counted"] > 0
    for f in ALL4:
        assert 2 * int(cells[f"sum_{f}"].sum()) == int(sites[f"sum_{f}"].sum()), f
        assert 2 * int(cells[f"linked_{f}"].sum()) == int(sites[f"linked_{f}"].sum()), f
    if bin_size == 137:
        assert stats["band"] >= 150 and stats["lds"] == 0
        monkeypatch.setenv("NGSLD_TEST_GRID_LDS_BYTES", "65536")
        eng = _engine(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True))
        try:
            _, one, _ = _check(eng, text, labels, bin_size, ld=("r2",))
        finally:
            eng.close()
        assert one["lds"] == 0
    if bin_size == 2000:
        assert stats["lds"] == 0  # (thirteen words x 3 row bins x a band of 16: 5 KB, beyond the 4 KiB that pay)
    if bin_size == 10 ** 9:
        assert stats["cells"] == 2 and stats["band"] == 1 and want["bin1"] == [0, 0] and want["chr"] == ["chr1", "chr2"]


def test_all_pairs_over_two_chromosomes():
    """No window: the band is the whole chromosome.  Rows across the two chromosomes are in the table (dist inf) and in no cell."""
    raw = synth.make_gl_numpy(300, 64, 864, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300, n_chr=2)
    _, stats, want, _ = _case(raw, chrs, pos, dict(extend_out=True), 2000, {})
    assert stats["pairs"] == 300 * 299 // 2 and stats["pairs_counted"] == 2 * (150 * 149 // 2)
    span = max(int(pos[k * 150 + 149]) // 2000 - int(pos[k * 150]) // 2000 + 1 for k in (0, 1))
    assert stats["band"] == span and max(b - a for a, b in zip(want["bin1"], want["bin2"])) == (span - 1) * 2000


def _knob_case(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    raw, chrs, pos, labels, text, _, _ = _one_input()
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True))
    try:
        a, sa, _ = _check(eng, text, labels, 2000, ld=ALL4, abs_value=False, linked_min=0.3)
        b, sb = eng.grid(labels, 2000, ld=ALL4, abs_value=False, linked_min=0.3)
        row_off, _ = eng.plan_rows()
    finally:
        eng.close()
    assert sa["chunks"] == sb["chunks"] and a.keys() == b.keys()
    for k in a:  # (two calls: the same bytes)
        assert a[k].tobytes() == b[k].tobytes(), k
    return a, sa, (chrs, pos, np.asarray(row_off))


def test_lds_global_and_small_chunks_give_the_same_arrays(monkeypatch):
    a0, s0, _ = _knob_case(monkeypatch, {"NGSLD_TEST_GRID_LDS_BYTES": "65536"})
    assert s0["lds"] == 1 and s0["chunks"] == 1
    a1, s1, _ = _knob_case(monkeypatch, {"NGSLD_TEST_GRID_LDS_BYTES": "0"})
    assert s1["lds"] == 0
    a2, s2, (chrs, pos, row_off) = _knob_case(monkeypatch, {"NGSLD_TEST_GRID_CHUNK_PAIRS": "3000", "NGSLD_TEST_GRID_LDS_BYTES": "65536"})
    assert s2["lds"] == 1 and s2["chunks"] > 5
    a3, s3, _ = _knob_case(monkeypatch, {"NGSLD_TEST_GRID_CHUNK_PAIRS": "3000", "NGSLD_TEST_GRID_LDS_BYTES": "0"})
    assert s3["lds"] == 0 and s3["chunks"] == s2["chunks"]
    a4, s4, _ = _knob_case(monkeypatch, {})  # (as shipped: 5 KB of window a tile is beyond the 4 KiB that pay)
    assert s4["lds"] == 0
    for a in (a1, a2, a3, a4):
        assert a.keys() == a0.keys()
        for k in a0:
            assert a[k].tobytes() == a0[k].tobytes(), k
    # the chunks of 3,000 pairs (run_record_chunks: consecutive rows while they fit): one begins inside a bin -- and every tile
    # of 16 rows is counted from there --, none at the chromosome change, which lies inside a chunk and inside a tile
    starts, r = [], 0
    while r < 600:
        starts.append(r)
        e = r + 1
        while e < 600 and row_off[e + 1] - row_off[r] <= 3000:
            e += 1
        r = e
    assert any(k > 0 and chrs[k] == chrs[k - 1] and pos[k] // 2000 == pos[k - 1] // 2000 for k in starts)
    k0 = max(k for k in starts if k <= 300)
    assert k0 < 300 and (300 - k0) % 16 != 0


def test_positions_with_repeated_values():
    """Two and three sites at one position (equal positions are fine: the gap is 0, the bin the same), some on a bin's break."""
    raw = synth.make_gl_numpy(400, 64, 964, depth=4.0)
    chrs, pos = synth.make_positions(400, 37, max_gap=300)
    pos = np.array(pos)
    pos[5::7] = pos[4::7][:len(pos[5::7])]
    pos[12::21] = pos[11::21][:len(pos[12::21])]
    k = 200
    pos[k:] += 2000 * (int(pos[k]) // 2000 + 1) - int(pos[k])  # (site k, and its twin k + 1 if it has one, exactly on a break)
    assert all(np.diff(pos) >= 0) and int(np.count_nonzero(np.diff(pos) == 0)) > 50 and int(pos[k]) % 2000 == 0
    _, stats, _, _ = _case(raw, chrs, pos, WIN, 2000, dict(ld=("r2", "D")))
    assert stats["pairs_counted"] > 0


def test_a_gap_of_megabases_inside_a_tile(monkeypatch):
    """3 Mb without a site in the middle of a tile.  A tile's window is sized for the row bins that 99 tiles in 100 span -- five
    here; of 1,600 rows only 15 begin a stretch of 16 that spans the gap.  The gap lies before site 808: rows 808 .. 815 of the
    tile 800 .. 815 lie some 3,000 bins beyond its window and add to global memory.  The same bytes as with every add there."""
    raw = synth.make_gl_numpy(1600, 8, 1264, depth=4.0)
    chrs, pos = synth.make_positions(1600, 37, max_gap=300)
    pos = np.array(pos)
    pos[808:] += 3_000_000
    out = []
    for env in ({}, {"NGSLD_TEST_GRID_LDS_BYTES": "0"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cells, stats, _, _ = _case(raw, chrs, pos, dict(max_kb_dist=5, extend_out=True), 1000, dict(ld=("r2", "Dp")))
        out.append(cells)
        assert stats["lds"] == (0 if env else 1) and stats["chunks"] == 1 and stats["bins"] > 3000 and stats["band"] <= 6
    assert int(pos[808]) // 1000 - int(pos[807]) // 1000 >= 3000
    assert all(out[0][k].tobytes() == out[1][k].tobytes() for k in out[0])


def test_tie_heavy_input_with_linked_min_on_a_printed_tie(monkeypatch):
    """300 sites of 8 called individuals, all pairs, D: thousands of values are exact "%f" ties (odd / 128 and the like).
    linked_min on the value the commonest tie prints, and on its other neighbour: the linked rows are those of the rule on the
    table, which has rows exactly on the threshold."""
    raw = np.eye(3)[synth.make_gl_numpy(300, 8, 15, depth=8.0).argmax(2)]
    chrs, pos = synth.make_positions(300, 48, max_gap=300)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, dict(extend_out=True))
    try:
        _, _, std, _ = eng.run()
        ties = is_tie(std["D"])
        assert int(ties.sum()) >= 1000
        vals, counts = np.unique(np.abs(std["D"][ties]), return_counts=True)
        q = micro(float(vals[np.argmax(counts)]))
        text = _tsv(eng, labels)
        on = sum(1 for f in (ln.split("\t") for ln in text.splitlines()[1:])
                 if abs(site_ref.micro(f[4]) or 0) == q and site_ref.micro(f[8]) is not None and site_ref.micro(f[9]) is not None)
        assert on > 0
        below = sum(1 for f in (ln.split("\t") for ln in text.splitlines()[1:])
                    if abs(site_ref.micro(f[4]) or 0) == q - 1 and site_ref.micro(f[8]) is not None and site_ref.micro(f[9]) is not None)
        linked = []
        for floor in (q, q + 1, q - 1):
            both = []
            for chunk in (None, "3000"):  # (one chunk, and sixteen)
                monkeypatch.delenv("NGSLD_TEST_GRID_CHUNK_PAIRS", raising=False)
                if chunk:
                    monkeypatch.setenv("NGSLD_TEST_GRID_CHUNK_PAIRS", chunk)
                cells, stats, _ = _check(eng, text, labels, 5000, ld=("D",), linked_min=floor / 10 ** 6)
                assert (stats["chunks"] > 5) == bool(chunk)
                both.append(cells)
            assert all(both[0][k].tobytes() == both[1][k].tobytes() for k in both[0])
            linked.append(int(both[0]["linked_D"].sum()))
    finally:
        eng.close()
    # the boundary rows are linked at q, not at q + 1; one unit lower the rows that print q - 1 join them
    assert linked[0] - linked[1] == on and linked[2] - linked[0] == below


# the cases of tests/test_gpu_analyses_by_family.py, one per family and item width (its un-called and masked twins of the
# multi-wavefront kernels left out); named here so that collecting this file imports nothing of that one
FAMILY_CASES = ["group16", "group32", "run10", "ab", "multi", "multi-ab", "stream_resident", "stream_plain"]


@pytest.mark.parametrize("name", FAMILY_CASES)
def test_one_windowed_case_under_every_pair_kernel_family(name, monkeypatch):
    """The pairs from the other kernel families (16- and 32-lane groups, the run kernel's last shape, the a/b and multi-wavefront
    kernels, both streaming kernels: items of 64 and of 16 candidates), forced the way tests/test_gpu_analyses_by_family.py
    forces them."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    import test_gpu_analyses_by_family as fam
    assert FAMILY_CASES == [k for k in fam.CASES if not k.endswith(("_mono", "_masked"))]
    inp_name, how, kernel, _, _ = fam.CASES[name]
    inp = fam._input(inp_name)
    eng = fam._new_engine(inp, how)
    try:
        fam._plan(eng, inp)
        assert eng.pair_kernel() == kernel
        text = fam._tsv(eng, inp)
        _, stats, _ = _check(eng, text, inp.labels, 2000, ld=("r2", "D"), abs_value=False, linked_min=0.3)
    finally:
        eng.close()
    assert stats["pairs"] == len(inp.keys) and stats["pairs_counted"] > 0 and stats["lds"] == 1


def test_the_result_goes_with_the_plan():
    raw = synth.make_gl_numpy(300, 16, 91, depth=4.0)
    chrs, pos = synth.make_positions(300, 91, max_gap=300)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        cells, st = eng.grid(labels, 2000, ld=("r2", "Dp"))
        n = np.zeros(max(int(st["cells"]), 1), dtype=np.uint64)
        got = C.c_uint64(0)
        assert eng._L.ngsld_grid_cells(eng._h, len(n), None, None, None, n.ctypes.data, C.byref(got)) == capi.OK
        assert got.value == st["cells"] > 0 and n.tobytes() == cells["n"].tobytes()
        assert eng._L.ngsld_grid_cells(eng._h, 0, None, None, None, None, C.byref(got)) == capi.OK and got.value == st["cells"]
        assert eng._L.ngsld_grid_get(eng._h, 5, len(n), None, None, None, None) == capi.ERR_INVALID  # (D was not chosen)
        assert eng._L.ngsld_grid_get(eng._h, 6, len(n), None, None, None, None) == capi.OK
        eng.plan(**WIN)
        assert eng._L.ngsld_grid_cells(eng._h, 0, None, None, None, None, C.byref(got)) == capi.ERR_INVALID
        assert eng._L.ngsld_grid_chromosomes(eng._h, 0, None, None) == capi.ERR_INVALID
    finally:
        eng.close()


def _refused(eng, labels, bin_size, code, *words, **kw):
    with pytest.raises(capi.NgsldError) as e:
        eng.grid(labels, bin_size, **kw)
    assert e.value.code == code and all(w in e.value.msg for w in words), (e.value.code, e.value.msg)


def test_refusals():
    raw = synth.make_gl_numpy(500, 16, 3, depth=4.0)
    chrs, pos = synth.make_positions(500, 37, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    U, I = capi.ERR_UNSUPPORTED, capi.ERR_INVALID
    eng = _engine(raw, chrs, pos, WIN)
    try:
        assert eng.grid(labels, 2000)[1]["cells"] > 0
        # positions: not digits, decreasing (equal ones are fine: test_positions_with_repeated_values)
        for bad in ("chr1:12a", "chr1:", "chr1", "chr1:-5", "chr1:1e3", "chr1:" + "9" * 20):
            _refused(eng, labels[:7] + [bad] + labels[8:], 2000, U, f'"{bad}"', "not plain decimal digits")
        swapped = labels[:10] + [labels[11], labels[10]] + labels[12:]
        _refused(eng, swapped, 2000, U, f'"{labels[10]}"', f'"{labels[11]}"', "below that of the site before it")
        # chromosomes: a name that begins two runs; labels against pos_dist, both ways
        again = labels[:250] + [f"chr1:{int(p)}" for p in pos[250:]]
        _refused(eng, again, 2000, U, f'"{again[250]}"', "but their distance is not finite")
        third = labels[:250] + [f"chr2:{int(p)}" for p in pos[250:400]] + [f"chr1:{int(p)}" for p in pos[400:]]
        _refused(eng, third, 2000, U, f'"{third[400]}"', "but their distance is finite")
        early = labels[:100] + [f"chr3:{int(p)}" for p in pos[100:250]] + labels[250:]
        _refused(eng, early, 2000, U, f'"{early[100]}"', f'"{early[99]}"', "but their distance is finite")
        # labels, parameters
        _refused(eng, None, 2000, I, "labels are NULL")
        _refused(eng, ["(null)"] * 500, 2000, I, "(null)")
        for b in (0, 2 ** 31, 2 ** 40):
            _refused(eng, labels, b, I, "bin_size")
        _refused(eng, labels, 2000, I, "linked_min is NaN", linked_min=math.nan)
        _refused(eng, labels, 2000, I, "min_maf is NaN", min_maf=math.nan)
        _refused(eng, labels, 2000, I, "max_kb_dist", max_kb_dist=math.nan)
        _refused(eng, labels, 2000, I, "max_kb_dist", max_kb_dist=-1.0)
        # the accumulators: a window of one base over a 20 kb window is tens of thousands of bins x a band of 20,001
        _refused(eng, labels, 1, U, "cells", "2 GiB", "a larger bin_size is needed")
        assert eng.grid(labels, 2000)[1]["cells"] > 0  # (a refusal leaves the context usable)
        p = capi.GridParams(C.sizeof(capi.GridParams) - 8, 8, 2000, math.inf, 0.0, 0.5, 1, 0)
        arr = (C.c_char_p * 500)(*[l.encode() for l in labels])
        assert eng._L.ngsld_grid(eng._h, C.byref(p), arr, None) == I and b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = capi.GridParams(C.sizeof(capi.GridParams), 8, 2000, math.inf, 0.0, 0.5, 1, 0)
        st = capi.GridStats()  # (struct_size not set)
        assert eng._L.ngsld_grid(eng._h, C.byref(p), arr, C.byref(st)) == I
        for fields in (0, 16):  # (an empty statistic set, an unknown one)
            p.fields = fields
            assert eng._L.ngsld_grid(eng._h, C.byref(p), arr, None) == I and b"fields" in eng._L.ngsld_last_error(eng._h)
        # a chromosome that is repeated further on: "a", "b", "a"
        two = [f"a:{int(p)}" for p in pos[:250]] + [f"b:{int(p)}" for p in pos[250:]]
        assert eng.grid(two, 2000)[1]["cells"] > 0
    finally:
        eng.close()
    chrs3, pos3 = synth.make_positions(300, 37, max_gap=300, n_chr=3)
    eng = _engine(synth.make_gl_numpy(300, 16, 3, depth=4.0), chrs3, pos3, WIN)
    try:
        aba = [f"{'a' if c != 'chr2' else 'b'}:{int(p)}" for c, p in zip(chrs3, pos3)]
        _refused(eng, aba, 2000, U, 'chromosome "a" begins a second time', f'"{aba[200]}"')
        gaps = np.full(300, 10.5)  # (positions no file holds: half a base between sites)
        eng.set_pos_dist(gaps)
        eng.plan(max_kb_dist=1, extend_out=True)
        one = [f"c:{10 * k + 10}" for k in range(300)]
        _refused(eng, one, 100, U, "integer position gaps", max_kb_dist=0.5)
        assert eng.grid(one, 100)[1]["pairs_counted"] > 0  # (no limit: only whether dist is finite matters)
    finally:
        eng.close()


def test_cli_grid_out(tmp_path):
    n_sites, n_ind = 500, 64
    raw = synth.make_gl_numpy(n_sites, n_ind, 97, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 97, max_gap=300, n_chr=2)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "20",
            "--extend_out"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, env=env: subprocess.run([*base, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300,  # noqa: E731
                                             env=env)
    gk = ["--grid_bin_size", "2000", "--grid_ld", "Dp,r2", "--grid_min_maf", "0.05", "--grid_linked_min", "0.3", "--grid_max_kb_dist", "15"]
    ref_kw = dict(ld=("Dp", "r2"), min_maf=0.05, linked_min=0.3, max_kb_dist=15.0)
    # --grid_out alone: the file, no TSV (not even on standard output)
    r = run("--grid_out", "s.tsv", *gk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> LD grid:" in r.stderr
    # a second run writes the table, and the file beside it: the table's bytes are those of a run without --grid_out
    r = run("--out", "t.tsv", "--grid_out", "s2.tsv", *gk)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--out", "t0.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    table = open(tmp_path / "t.tsv", "rb").read()
    assert table == open(tmp_path / "t0.tsv", "rb").read() and len(table) > 100_000
    want = grid_ref.grid_file(table.decode(), _labels(chrs, pos), 2000, **ref_kw)
    assert len(want.splitlines()) > 100 and "chr2\t" in want
    assert open(tmp_path / "s.tsv").read() == want
    assert open(tmp_path / "s2.tsv").read() == want
    # signed values, and beside the other analyses
    r = run("--grid_out", "s3.tsv", "--grid_bin_size=700", "--grid_ld", "D", "--grid_signed", "--decay_out", "b.tsv", "--prune_out", "k.txt",
            "--site_out", "u.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "s3.tsv").read() == grid_ref.grid_file(table.decode(), _labels(chrs, pos), 700, ld=("D",), abs_value=False)
    assert all(os.path.getsize(tmp_path / f) > 0 for f in ("b.tsv", "k.txt", "u.tsv"))
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--grid_out", "s5.tsv", "--grid_bin_size", "2000", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--grid_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "s5.tsv")
