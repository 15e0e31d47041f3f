"""The LD decay map on the device (ngsld_decay_map, Engine.decay_map, the binary's --dmap_* flags) against tests/decay_map_ref.py
-- decay_ref, the restatement of fit_LDdecay.R's binning, applied to each group's rows -- on the same engine's own TSV
(run_text).  Counts must be equal and every mean must be the double nearest to the exact mean of the printed decimals; between
launch shapes, chunks and kernel forms the arrays must be the same bytes.  No tolerances.

The input is 221 sites in three chromosomes of 150, 1 and 70: the long one gives rows of more than 64 candidates (several work
items a row), the middle one has no pair of its own.  Every engine and its TSV are made once and shared."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import decay_map_ref
import decay_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
SIZES = (("chrA", 150), ("chrB", 1), ("chrC", 70))
N_SITES = sum(n for _, n in SIZES)
W = 4000  # chrA spans some 22 kb: at least five windows, and pairs further apart than a window
KNOBS = ("DMAP_CHUNK_PAIRS", "DMAP_LDS_BYTES", "RECORD_SLICE_ITEMS", "SUM_WRAP_LIMIT")


def _positions():
    chrs, pos = [], []
    for k, (name, n) in enumerate(SIZES):
        _, p = synth.make_positions(n, 41 + k, max_gap=300)
        chrs += [name] * n
        pos += [int(x) for x in p]
    return chrs, np.array(pos, dtype=np.int64)


CHRS, POS = _positions()
LABELS = [f"{c}:{int(p)}" for c, p in zip(CHRS, POS)]
# name: (n_ind, synth kw, plan kw, geno kw)
INPUTS = {
    "n64_all": (64, {}, dict(extend_out=True), None),
    "n16_win": (16, {}, dict(max_kb_dist=10, extend_out=True), None),
    "mono64": (64, dict(mono_frac=0.2), dict(extend_out=True), None),
    "call16": (16, dict(mono_frac=0.2), dict(max_kb_dist=10, extend_out=True), dict(call_geno=(0.1, 0.9))),
}
_made = {}


def _raw(name):
    n_ind, skw, _, _ = INPUTS[name]
    return synth.make_gl_numpy(N_SITES, n_ind, 900 + n_ind, depth=4.0, **skw)


def _new_engine(raw, chrs, pos, plan_kw, geno_kw):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


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
        _, _, plan_kw, geno_kw = INPUTS[name]
        eng = _new_engine(_raw(name), CHRS, POS, plan_kw, geno_kw)
        eng.set_text_output(LABELS)
        text, fallbacks = eng.run_text()
        assert fallbacks == 0
        _made[name] = (eng, text.decode())
    return _made[name]


def _same(bins, want, ld):
    """tests/test_gpu_decay.py's comparison: dist and n equal, every mean bit for bit float(Fraction)."""
    chosen = [f for f in decay_ref.FIELDS if f in ld]
    assert len(bins["dist"]) == len(want), (len(bins["dist"]), len(want))
    assert [float(x) for x in bins["dist"]] == [w[0] for w in want]
    assert [int(x) for x in bins["n"]] == [w[1] for w in want]
    for f in chosen:
        got = bins[f]
        exp = np.array([float(w[2][f]) for w in want])
        bad = np.nonzero(got.view(np.int64) != exp.view(np.int64))[0]
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _same_map(groups, want, ld, names=None):
    assert [(g["chr"], g["win_start"]) for g in groups] == [((names or {}).get(c, c), w) for c, w, _ in want]
    for g, (_, _, bins) in zip(groups, want):
        _same(g, bins, ld)


def _bytes(groups):
    return [(g["chr"], g["win_start"]) + tuple((k, v.tobytes()) for k, v in g.items() if k not in ("chr", "win_start")) for g in groups]


def _check(name, labels=LABELS, names=None, **kw):
    eng, text = _input(name)
    groups, stats = eng.decay_map(labels, **kw)
    want = decay_map_ref.decay_map(text, **kw)
    _same_map(groups, want, kw.get("ld", ("r2",)), names)
    assert stats["groups"] == len(want) > 0 and stats["bins"] == sum(len(b) for _, _, b in want)
    assert stats["pairs_counted"] == sum(w[1] for _, _, b in want for w in b) > 0
    return groups, stats, want


# ---- 1. per chromosome ----
@pytest.mark.parametrize("name", ["n64_all", "n16_win"])
def test_per_chromosome_equals_the_script_per_file(name):
    groups, stats, want = _check(name)
    assert [g["chr"] for g in groups] == ["chrA", "chrC"] and stats["group_slots"] == 3  # (the one-site chromosome: no group)
    assert all(g["win_start"] == 0 for g in groups)
    # without labels: the same bins under the chromosomes' ordinals
    eng, _ = _input(name)
    by_ordinal, _ = eng.decay_map(None)
    assert [g["chr"] for g in by_ordinal] == ["1", "3"]
    assert [b[2:] for b in _bytes(by_ordinal)] == [b[2:] for b in _bytes(groups)]
    # each group is ngsld_decay's answer on an engine that holds only that chromosome's sites
    n_ind, _, plan_kw, geno_kw = INPUTS[name]
    raw = _raw(name)
    for g in groups:
        sl = [k for k, c in enumerate(CHRS) if c == g["chr"]]
        sub = _new_engine(raw[sl], [CHRS[k] for k in sl], POS[sl], plan_kw, geno_kw)
        try:
            bins, _ = sub.decay()
        finally:
            sub.close()
        assert set(bins) | {"chr", "win_start"} == set(g)
        for k in bins:
            assert bins[k].tobytes() == g[k].tobytes(), (g["chr"], k)


# ---- 2. windows ----
@pytest.mark.parametrize("name", ["n64_all", "n16_win"])
def test_windows_equal_the_script_per_file(name):
    groups, stats, want = _check(name, window=W)
    assert sum(1 for g in groups if g["chr"] == "chrA") >= 4
    assert all(g["win_start"] % W == 0 for g in groups)
    _, text = _input(name)
    _, parts, _ = decay_map_ref.split_rows(text, W)
    outside = 0  # rows whose midpoint's window holds neither site
    for (c, w), rows in parts.items():
        for ln in rows:
            p1, p2 = (int(x.split(":")[1]) for x in ln.split("\t")[:2])
            outside += w not in (p1 // W, p2 // W)
    assert outside > 0


def test_a_window_beyond_every_position_is_the_chromosome():
    eng, _ = _input("n64_all")
    by_chr, _ = eng.decay_map(LABELS)
    wide, stats = eng.decay_map(LABELS, window=2 ** 31 - 1)
    assert int(POS.max()) < 2 ** 31 - 1 and stats["group_slots"] == 3
    assert _bytes(wide) == _bytes(by_chr)


# ---- 3. every statistic, NaN rows, printed ties, min_maf, a strict limit ----
def _dist_in_table(text):
    """A dist of the table that max_kb_dist can state exactly."""
    dists = sorted({int(ln.split("\t")[2]) for ln in text.splitlines() if ln.split("\t")[2].isdigit()})
    return next(d for d in dists[len(dists) // 2:] if (d / 1000) * 1000 == d)


@pytest.mark.parametrize("name,window", [("mono64", 0), ("mono64", W), ("call16", W), ("call16", 0)])
def test_all_statistics_with_filters(name, window):
    _, text = _input(name)
    d = _dist_in_table(text)
    assert f"\t{d}\t" in text
    _, _, want = _check(name, window=window, ld=ALL4, min_maf=0.1, max_kb_dist=d / 1000, bin_size=33.3)
    assert max(w[0] for _, _, b in want for w in b) < d  # (strict: the rows at d are out)
    _check(name, window=window, ld=ALL4)
    # the monomorphic sites give rows with a NaN or an inf, which drop out of every statistic (the table has no header line)
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert any(r[0].split(":")[0] == r[1].split(":")[0] and any(not math.isfinite(float(x)) for x in r[3:7]) for r in rows)


# ---- 4. the groups add up to the pooled bins ----
@pytest.mark.parametrize("window", [0, W])
def test_groups_add_up_to_ngsld_decay(window):
    eng, _ = _input("n16_win")
    kw = dict(ld=("D", "r2"), bin_size=100)
    pooled, pst = eng.decay(**kw)
    groups, st = eng.decay_map(LABELS, window=window, **kw)
    n = {}
    for g in groups:
        for dist, cnt in zip(g["dist"], g["n"]):
            n[float(dist)] = n.get(float(dist), 0) + int(cnt)
    assert sorted(n) == [float(x) for x in pooled["dist"]]
    assert [n[float(x)] for x in pooled["dist"]] == [int(x) for x in pooled["n"]]
    assert st["pairs_counted"] == pst["pairs_counted"] == sum(n.values()) and st["pairs"] == pst["pairs"]


# ---- 5. chunks and slices, 6. the two kernel forms ----
@pytest.mark.parametrize("window", [0, W])
def test_chunks_slices_and_forms_give_the_same_bytes(monkeypatch, window):
    eng, _ = _input("n64_all")
    kw = dict(window=window, ld=ALL4)
    g0, s0 = eng.decay_map(LABELS, **kw)
    assert s0["lds"] == 1 and s0["chunks"] == 1
    monkeypatch.setenv("NGSLD_TEST_DMAP_LDS_BYTES", "0")
    g1, s1 = eng.decay_map(LABELS, **kw)
    assert s1["lds"] == 0 and s1["chunks"] == 1
    monkeypatch.setenv("NGSLD_TEST_DMAP_CHUNK_PAIRS", str(s0["pairs"] // 10))
    monkeypatch.setenv("NGSLD_TEST_RECORD_SLICE_ITEMS", "7")
    g2, s2 = eng.decay_map(LABELS, **kw)
    assert s2["lds"] == 0 and s2["chunks"] > 5
    monkeypatch.delenv("NGSLD_TEST_DMAP_LDS_BYTES")
    g3, s3 = eng.decay_map(LABELS, **kw)
    assert s3["lds"] == 1 and s3["chunks"] == s2["chunks"]
    for g in (g1, g2, g3):
        assert _bytes(g) == _bytes(g0)
    for s in (s1, s2, s3):
        assert {k: v for k, v in s.items() if not k.endswith("_ms") and k not in ("lds", "chunks")} == \
               {k: v for k, v in s0.items() if not k.endswith("_ms") and k not in ("lds", "chunks")}


# ---- 7. the guard of the sums ----
def _getters_refuse(eng):
    L, h = eng._L, eng._h
    n = C.c_uint64(7)
    for rc in (L.ngsld_decay_map_chromosomes(h, 0, None, C.byref(n)), L.ngsld_decay_map_groups(h, 0, None, None, None, None, C.byref(n)),
               L.ngsld_decay_map_bins(h, 0, None, None, None, C.byref(n))):
        assert rc == capi.ERR_INVALID
        assert L.ngsld_last_error(h).decode() == "no ngsld_decay_map result (it goes with the next ngsld_plan or ngsld_set_*)"
    assert n.value == 7


@pytest.mark.parametrize("window", [0, W])
def test_sum_guard_at_its_limit(monkeypatch, window):
    """max |q| over the counted rows times the planned pairs is refused, one unit more is accepted (record_pass.h)."""
    eng, text = _input("n16_win")
    ld = ("D", "Dp")
    kw = dict(window=window, ld=ld)
    g0, s0 = eng.decay_map(LABELS, **kw)
    M = 0
    for ln in text.splitlines():  # (no header line: ngsLD's column layout)
        f = ln.split("\t")
        vals = [float(f[decay_ref.COLUMNS.index(s)]) for s in ld]
        if f[0].split(":")[0] == f[1].split(":")[0] and all(math.isfinite(v) for v in vals):
            M = max(M, max(int(round(abs(v) * 1e6)) for v in vals))
    T = M * s0["pairs"]
    assert M > 0
    monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(T))
    with pytest.raises(capi.NgsldError) as e:
        eng.decay_map(LABELS, **kw)
    assert e.value.code == capi.ERR_UNSUPPORTED and "too large to sum exactly" in e.value.msg and f"{s0['pairs']} pairs" in e.value.msg
    _getters_refuse(eng)
    monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(T + 1))
    g1, _ = eng.decay_map(LABELS, **kw)
    assert _bytes(g1) == _bytes(g0)
    monkeypatch.setenv("NGSLD_TEST_SUM_WRAP_LIMIT", str(2 ** 63))  # (tracking on, the shipped limit)
    g2, _ = eng.decay_map(LABELS, **kw)
    assert _bytes(g2) == _bytes(g0)


# ---- 8. refusals ----
def _raw_call(eng, labels=LABELS, struct_size=None, fields=8, bin_size=250.0, max_kb_dist=math.inf, min_maf=0.0, window=0):
    p = capi.DecayMapParams(C.sizeof(capi.DecayMapParams) if struct_size is None else struct_size, fields, bin_size, max_kb_dist,
                            min_maf, window)
    st = capi.DecayMapStats()
    st.struct_size = C.sizeof(capi.DecayMapStats)
    arr = None if labels is None else (C.c_char_p * len(labels))(*[l.encode() for l in labels])
    rc = eng._L.ngsld_decay_map(eng._h, C.byref(p), arr, C.byref(st))
    return rc, eng._L.ngsld_last_error(eng._h).decode()


def _with(k, label):
    return LABELS[:k] + [label] + LABELS[k + 1:]


SPREAD = [f"{c}:{(k + 1) * 4_500_000}" for k, c in enumerate(CHRS)]  # positions up to 10^9
REFUSALS = {
    # name: (keywords of _raw_call, code, part of the message)
    "window_without_labels": (dict(labels=None, window=W), capi.ERR_INVALID, "LD decay map: a window needs positions: the labels are NULL"),
    "null_label": (dict(labels=_with(5, "(null)"), window=W), capi.ERR_INVALID, "LD decay map: a window needs positions: a label is \"(null)\""),
    "position_not_decimal": (dict(labels=_with(5, "chrA:12x"), window=W), capi.ERR_UNSUPPORTED,
                             "LD decay map: the position of label \"chrA:12x\" is not plain decimal digits"),
    "position_2^62": (dict(labels=_with(149, f"chrA:{2 ** 62}"), window=W), capi.ERR_UNSUPPORTED, "LD decay map: the position of label"),
    "positions_decrease": (dict(labels=_with(7, "chrA:1"), window=W), capi.ERR_UNSUPPORTED,
                           "LD decay map: the position of site \"chrA:1\" is below that of the site before it"),
    "window_2^31": (dict(window=2 ** 31), capi.ERR_INVALID, "decay map window must be 0 (per chromosome) or an integer in [1, 2^31)"),
    "bin_size_1": (dict(bin_size=1.0), capi.ERR_INVALID, "decay map bin_size must be a finite number > 1"),
    "fields_0": (dict(fields=0), capi.ERR_INVALID, "decay map fields must be a non-empty mask"),
    "fields_16": (dict(fields=16), capi.ERR_INVALID, "decay map fields must be a non-empty mask"),
    "min_maf_nan": (dict(min_maf=math.nan), capi.ERR_INVALID, "decay map min_maf is NaN"),
    "struct_size": (dict(struct_size=8), capi.ERR_INVALID, "ngsld_decay_map_params: struct_size must be sizeof(ngsld_decay_map_params)"),
    "accumulator_cap": (dict(labels=SPREAD, window=1, bin_size=2.0), capi.ERR_UNSUPPORTED, "a larger window or bin_size is needed"),
}


def test_refusals_leave_the_store_empty_and_decay_alone():
    eng, _ = _input("n16_win")
    pooled, _ = eng.decay(ld=("D", "r2"))
    good, _ = eng.decay_map(LABELS, window=W)
    for name, (kw, code, part) in REFUSALS.items():
        eng.decay_map(LABELS, window=W)  # (a filled store, which the refusal must empty)
        rc, msg = _raw_call(eng, **kw)
        assert rc == code and part in msg, (name, rc, msg)
        if name == "accumulator_cap":
            assert "group slots x" in msg and "bins x" in msg, msg
        _getters_refuse(eng)
        nb = C.c_uint64(0)  # ngsld_decay's store is as it was
        dist = np.zeros(len(pooled["dist"]))
        assert eng._L.ngsld_decay_bins(eng._h, len(dist), dist.ctypes.data, None, None, C.byref(nb)) == capi.OK
        assert nb.value == len(pooled["dist"]) and dist.tobytes() == pooled["dist"].tobytes(), name
    again, _ = eng.decay_map(LABELS, window=W)  # the context is usable
    assert _bytes(again) == _bytes(good)


def test_getters_before_a_call_and_after_a_new_plan():
    raw = _raw("n16_win")[:40]
    eng = _new_engine(raw, CHRS[:40], POS[:40], dict(extend_out=True), None)
    try:
        _getters_refuse(eng)
        groups, _ = eng.decay_map(LABELS[:40], window=W)
        assert len(groups) > 0
        n = C.c_uint64(0)
        assert eng._L.ngsld_decay_map_groups(eng._h, 0, None, None, None, None, C.byref(n)) == capi.OK and n.value == len(groups)
        eng.plan(max_kb_dist=5)
        _getters_refuse(eng)
        assert len(eng.decay_map(LABELS[:40], window=W)[0]) > 0
    finally:
        eng.close()


# ---- 9. the binary ----
def _write_map(groups, ld):
    chosen = [f for f in decay_ref.FIELDS if f in ld]
    out = "chr\twin_start\tdist\tn" + "".join("\t" + f for f in chosen) + "\n"
    for g in groups:
        for i in range(len(g["dist"])):
            out += f"{g['chr']}\t{g['win_start']}\t" + "%.15g\t%d" % (g["dist"][i], g["n"][i]) + "".join("\t%.17g" % g[f][i] for f in chosen) + "\n"
    return out


def _write_fit(groups, ld, min_bins=3):
    out = "chr\twin_start\tLD\tDecayRate\tLDmax\tLDmin\tSSE\tn_bins\n"
    fits = {f: capi.decay_map_fit(groups, f, min_bins=min_bins) for f in decay_ref.FIELDS if f in ld and f != "D"}
    for k, g in enumerate(groups):
        for f, fit in fits.items():
            r = fit[k]
            tail = "\tNA\tNA\tNA\tNA\t%d" % len(g["dist"]) if r is None else "\t%.17g\t%.17g\t%.17g\t%.17g\t%d" % (
                r["rate"], r["ld_max"], r["ld_min"], r["sse"], r["n_bins"])
            out += f"{g['chr']}\t{g['win_start']}\t{f}" + tail + "\n"
    return out


def test_cli_dmap_files(tmp_path):
    name = "n16_win"
    n_ind = INPUTS[name][0]
    eng, _ = _input(name)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    _raw(name).astype("<f8").tofile(g)
    synth.write_pos(p, CHRS, POS)
    geno = ["--geno", g, "--n_ind", str(n_ind), "--n_sites", str(N_SITES), "--max_kb_dist", "10", "--extend_out"]
    base = [capi.CLI_PATH, *geno, "--pos", p]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, cmd=base: subprocess.run([*cmd, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)  # noqa: E731
    ld = ("Dp", "r2")
    dk = ["--dmap_ld", "Dp,r2", "--dmap_bin_size", "500", "--dmap_min_maf", "0.05"]
    kw = dict(ld=ld, bin_size=500, min_maf=0.05)
    # per chromosome and per window, no --out: no TSV, the files are the Python writer's
    for tag, extra, window in (("c", [], 0), ("w", ["--dmap_window", str(W)], W)):
        r = run("--dmap_out", f"m{tag}.tsv", "--dmap_fit", f"f{tag}.tsv", *dk, *extra)
        assert r.returncode == 0 and r.stdout == "", r.stderr[-2000:]
        groups, _ = eng.decay_map(LABELS, window=window, **kw)
        assert open(tmp_path / f"m{tag}.tsv").read() == _write_map(groups, ld)
        assert open(tmp_path / f"f{tag}.tsv").read() == _write_fit(groups, ld)
    # a group below --dmap_fit_min_bins gets its NA line
    r = run("--dmap_fit", "f5.tsv", "--dmap_window", str(W), "--dmap_fit_min_bins", "12", *dk)
    assert r.returncode == 0, r.stderr[-2000:]
    fit12 = open(tmp_path / "f5.tsv").read()
    assert fit12 == _write_fit(groups, ld, min_bins=12)
    na = [ln for ln in fit12.splitlines() if "\tNA\tNA\tNA\tNA\t" in ln]
    assert 0 < len(na) < len(fit12.splitlines()) - 1
    # with --decay_out: both files, the decay family's flags are its own (the prefix trap), its bytes those of the flag alone
    r = run("--dmap_out", "m2.tsv", "--decay_out", "d2.tsv", "--decay_ld", "Dp,r2", "--decay_bin_size", "500", "--decay_min_maf", "0.05", *dk)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--decay_out", "d1.tsv", "--decay_ld", "Dp,r2", "--decay_bin_size", "500", "--decay_min_maf", "0.05")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "d2.tsv").read() == open(tmp_path / "d1.tsv").read()
    assert open(tmp_path / "m2.tsv").read() == open(tmp_path / "mc.tsv").read()
    # the tails of --dmap_out's lines are --decay_out's format: one chromosome's lines are that chromosome's --decay_out
    pooled = [ln.split("\t") for ln in open(tmp_path / "d1.tsv").read().splitlines()]
    lines = [ln.split("\t") for ln in open(tmp_path / "mc.tsv").read().splitlines()]
    assert lines[0][2:] == pooled[0] and all(len(ln) == len(pooled[0]) + 2 for ln in lines)
    # refused before any device is touched
    no_pos = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(N_SITES), "--max_kb_dist", "0"]  # (a limit needs --pos itself)
    r = run("--dmap_out", "x.tsv", "--dmap_window", str(W), cmd=no_pos)
    assert r.returncode == 255 and "--dmap_window needs positions: it cannot run without --pos" in r.stderr, r.stderr[-1000:]
    r = run("--dmap_out", "x.tsv", "--devices", "0,1")
    assert r.returncode == 255 and "--dmap_out runs on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "x.tsv")
