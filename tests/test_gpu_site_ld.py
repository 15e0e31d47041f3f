"""Per-site LD summaries on the device (ngsld_site_ld, Engine.site_ld, the binary's --site_* flags) against tests/site_ref.py
-- the rule of SITES.md in plain Python -- applied to the same engine's own TSV (run_text).  Every n, sum, max and linked of
every site must be equal as integers and every mean bit for bit: nothing sampled, no tolerance.

GPU time of this file on one MI355X: see SITES.md ("What the tests cost")."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import site_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

NA_MAX = np.iinfo(np.int64).min


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _labels(chrs, pos):
    return [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]


def _tsv(eng, chrs, pos):
    eng.set_text_output(_labels(chrs, pos))
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _same(sites, want, ld):
    chosen = [f for f in site_ref.FIELDS if f in ld]
    assert set(sites) == {"n"} | {f"{w}_{f}" for f in chosen for w in ("sum", "max", "linked", "mean")}
    assert [int(x) for x in sites["n"]] == want["n"]
    for f in chosen:
        assert [int(x) for x in sites[f"sum_{f}"]] == want[f"sum_{f}"], f
        assert [int(x) for x in sites[f"linked_{f}"]] == want[f"linked_{f}"], f
        assert [None if x == NA_MAX else int(x) for x in sites[f"max_{f}"]] == want[f"max_{f}"], f
        exp = np.array([math.nan if m is None else m for m in want[f"mean_{f}"]])
        got = sites[f"mean_{f}"]
        assert np.array_equal(np.isnan(got), np.isnan(exp)), f
        ok = ~np.isnan(exp)
        bad = np.nonzero(got[ok].view(np.int64) != exp[ok].view(np.int64))[0]
        assert len(bad) == 0, (f, bad[:5], got[ok][bad[:5]], exp[ok][bad[:5]])


def _case(raw, chrs, pos, plan_kw, site_kw, geno_kw=None):
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, chrs, pos)
        sites, stats = eng.site_ld(**site_kw)
    finally:
        eng.close()
    want = site_ref.site_ld(text, _labels(chrs, pos), **site_kw)
    _same(sites, want, site_kw.get("ld", ("r2",)))
    assert stats["pairs"] == sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))
    assert stats["pairs_counted"] * 2 == sum(want["n"]) and stats["sites_with_pairs"] == sum(1 for x in want["n"] if x)
    print(f"pairs {stats['pairs']} counted {stats['pairs_counted']} sites {stats['sites_with_pairs']} lds {stats['lds']} "
          f"chunks {stats['chunks']} pairs_ms {stats['pairs_ms']:.2f} site_ms {stats['site_ms']:.3f} total_ms {stats['total_ms']:.2f}")
    return sites, stats, want, text


# extend_out everywhere: the restatement applies the maf filter where the TSV has maf1 / maf2
WIN = dict(max_kb_dist=20, extend_out=True)
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, site kw, geno kw)
    "n8_window": (500, 8, {}, 1, WIN, {}, None),
    "n64_window": (500, 64, {}, 1, WIN, {}, None),
    "n500_window": (400, 500, {}, 1, WIN, {}, None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=30, min_maf=0.1, rnd_sample=0.6, seed=7, extend_out=True), {}, None),
    "site_min_maf": (500, 64, {}, 1, WIN, dict(min_maf=0.2), None),
    "all_four": (400, 64, {}, 1, WIN, dict(ld=ALL4, linked_min=0.2), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, dict(ld=ALL4), None),
    "call_geno": (500, 64, {}, 1, WIN, dict(ld=("r2", "Dp")), dict(call_geno=(0.1, 0.9))),
    "max_snp_dist": (500, 64, {}, 2, dict(max_snp_dist=40, extend_out=True), dict(ld=("Dp", "r2")), None),
    "signed_D_Dp": (400, 64, {}, 1, WIN, dict(ld=("D", "Dp"), abs_value=False, linked_min=0.1), None),
    "kb_limit_inside_the_window": (400, 64, {}, 1, WIN, dict(max_kb_dist=7.5, ld=("D", "r2")), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_site_ld_equals_the_rule_on_own_tsv(name):
    n_sites, n_ind, skw, n_chr, plan_kw, site_kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 500 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 37, max_gap=300, n_chr=n_chr)
    _, stats, want, text = _case(raw, chrs, pos, plan_kw, site_kw, geno_kw)
    assert stats["pairs_counted"] > 0 and stats["lds"] == 1
    if name == "uncalled_mono":
        assert stats["pairs_counted"] < stats["pairs"]  # (NaN rows)
    if name == "signed_D_Dp":
        # (the table holds negative D: the signed sums are not the absolute ones)
        assert want["sum_D"] != site_ref.site_ld(text, _labels(chrs, pos), **{**site_kw, "abs_value": True})["sum_D"]


def test_all_pairs_over_two_chromosomes_take_the_global_path(monkeypatch):
    """No window: a row reaches every later site and the span of a tile does not fit the LDS it may use (4 KB here; 64 KB
    hold ~2,000 sites of one statistic).  Rows across the two chromosomes are in the table (dist inf) and never counted."""
    monkeypatch.setenv("NGSLD_TEST_SITE_LDS_BYTES", "4096")
    raw = synth.make_gl_numpy(300, 64, 864, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300, n_chr=2)
    _, stats, _, _ = _case(raw, chrs, pos, dict(extend_out=True), {})
    assert stats["lds"] == 0 and stats["pairs"] == 300 * 299 // 2
    assert stats["pairs_counted"] == 2 * (150 * 149 // 2)


def test_all_pairs_with_four_statistics_leave_the_lds_budget():
    """The global path at the budget the library ships with: 700 sites, no window, four statistics -- 13 words x 700 sites x 8 B
    is 72.8 KB, beyond the 64 KiB a tile may use."""
    raw = synth.make_gl_numpy(700, 16, 716, depth=4.0)
    chrs, pos = synth.make_positions(700, 37, max_gap=300)
    _, stats, _, _ = _case(raw, chrs, pos, dict(extend_out=True), dict(ld=ALL4))
    assert stats["lds"] == 0 and stats["pairs_counted"] == 700 * 699 // 2


def test_limit_on_a_present_dist():
    """max_kb_dist * 1000 equal to a dist the TSV holds: the rule is not strict, those rows are in."""
    raw = synth.make_gl_numpy(300, 64, 61, depth=4.0)
    chrs, pos = synth.make_positions(300, 61, max_gap=300)
    d = next(float(pos[k] - pos[0]) for k in range(60, 300) if (float(pos[k] - pos[0]) / 1000) * 1000 == float(pos[k] - pos[0]))
    eng = _engine(raw, chrs, pos, dict(extend_out=True))
    try:
        text = _tsv(eng, chrs, pos)
        sites, _ = eng.site_ld(max_kb_dist=d / 1000)
    finally:
        eng.close()
    assert f"\t{int(d)}\t" in text  # (the limit is a dist of the table)
    labels = _labels(chrs, pos)
    want = site_ref.site_ld(text, labels, max_kb_dist=d / 1000)
    _same(sites, want, ("r2",))
    on_limit = sum(1 for ln in text.splitlines() if ln.split("\t")[2] == str(int(d)))
    below = site_ref.site_ld(text, labels, max_kb_dist=(d - 0.5) / 1000)
    assert on_limit > 0 and sum(want["n"]) == sum(below["n"]) + 2 * on_limit


def _knob_case(monkeypatch, env):
    for k in ("NGSLD_TEST_SITE_LDS_BYTES", "NGSLD_TEST_SITE_CHUNK_PAIRS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    raw = synth.make_gl_numpy(600, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(600, 71, max_gap=300)
    return _case(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True), dict(ld=ALL4, abs_value=False, linked_min=0.3))[:3]


def test_lds_global_and_small_chunks_give_the_same_arrays(monkeypatch):
    a0, s0, _ = _knob_case(monkeypatch, {})
    assert s0["lds"] == 1 and s0["chunks"] == 1
    a1, s1, _ = _knob_case(monkeypatch, {"NGSLD_TEST_SITE_LDS_BYTES": "0"})
    assert s1["lds"] == 0
    a2, s2, _ = _knob_case(monkeypatch, {"NGSLD_TEST_SITE_CHUNK_PAIRS": "3000"})
    assert s2["lds"] == 1 and s2["chunks"] > 5
    a3, s3, _ = _knob_case(monkeypatch, {"NGSLD_TEST_SITE_CHUNK_PAIRS": "3000", "NGSLD_TEST_SITE_LDS_BYTES": "0"})
    assert s3["lds"] == 0 and s3["chunks"] == s2["chunks"]
    for a in (a1, a2, a3):
        assert a.keys() == a0.keys()
        for k in a0:
            assert a[k].tobytes() == a0[k].tobytes(), k


def test_linked_is_the_degree_in_the_pruning_graph():
    """One statistic, no maf filter: a site's linked partners are its edges in the graph ngsld_prune builds with the same field,
    distance limit and min_weight = linked_min, weight type a -- every edge has two ends."""
    raw = synth.make_gl_numpy(500, 64, 1064, depth=4.0)
    chrs, pos = synth.make_positions(500, 37, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        sites, _ = eng.site_ld(ld=("r2",), max_kb_dist=12.0, linked_min=0.2)
        _, pst = eng.prune(_labels(chrs, pos), field=7, max_kb_dist=12.0, min_weight=0.2, weight_type="a")
    finally:
        eng.close()
    assert pst["edges"] > 0 and int(sites["linked_r2"].sum()) == 2 * pst["edges"]


def test_two_calls_give_the_same_bits_and_the_result_goes_with_the_plan():
    raw = synth.make_gl_numpy(500, 64, 91, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 91, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        a, sa = eng.site_ld(ld=ALL4)
        b, sb = eng.site_ld(ld=ALL4)
        n = np.zeros(500, dtype=np.uint64)
        assert eng._L.ngsld_site_ld_get(eng._h, 7, n.ctypes.data, None, None, None, None) == capi.OK and n.tobytes() == a["n"].tobytes()
        eng.site_ld(ld=("r2",))
        assert eng._L.ngsld_site_ld_get(eng._h, 5, n.ctypes.data, None, None, None, None) == capi.ERR_INVALID  # (D was not chosen)
        eng.plan(**WIN)
        assert eng._L.ngsld_site_ld_get(eng._h, 7, n.ctypes.data, None, None, None, None) == capi.ERR_INVALID
    finally:
        eng.close()
    assert sa["pairs_counted"] == sb["pairs_counted"] > 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals():
    raw = synth.make_gl_numpy(100, 16, 3, depth=4.0)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        gaps = np.full(100, 10.5)  # (positions no file holds: half a base between sites)
        eng.set_pos_dist(gaps)
        eng.plan(max_kb_dist=1, extend_out=True)
        with pytest.raises(capi.NgsldError) as e:
            eng.site_ld(max_kb_dist=0.5)
        assert e.value.code == capi.ERR_UNSUPPORTED and "integer position gaps" in e.value.msg
        sites, _ = eng.site_ld()  # (no limit: only whether dist is finite matters)
        assert int(sites["n"].sum()) > 0
        p = capi.SiteLdParams(C.sizeof(capi.SiteLdParams) - 8, 8, math.inf, 0.0, 0.5, 1, 0)
        assert eng._L.ngsld_site_ld(eng._h, C.byref(p), None) == capi.ERR_INVALID
        assert b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = capi.SiteLdParams(C.sizeof(capi.SiteLdParams), 8, math.inf, 0.0, 0.5, 1, 0)
        st = capi.SiteLdStats()  # (struct_size not set)
        assert eng._L.ngsld_site_ld(eng._h, C.byref(p), C.byref(st)) == capi.ERR_INVALID
        p.fields = 16
        assert eng._L.ngsld_site_ld(eng._h, C.byref(p), None) == capi.ERR_INVALID
    finally:
        eng.close()


def test_cli_site_out(tmp_path):
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
    sk = ["--site_ld", "Dp,r2", "--site_min_maf", "0.05", "--site_linked_min", "0.3", "--site_max_kb_dist", "15"]
    ref_kw = dict(ld=("Dp", "r2"), min_maf=0.05, linked_min=0.3, max_kb_dist=15.0)
    # --site_out alone: the file, no TSV (not even on standard output)
    r = run("--site_out", "s.tsv", *sk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> Site LD:" in r.stderr
    # a second run writes the table, and the file beside it: the table's bytes are those of a run without --site_out
    r = run("--out", "t.tsv", "--site_out", "s2.tsv", *sk)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--out", "t0.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    table = open(tmp_path / "t.tsv", "rb").read()
    assert table == open(tmp_path / "t0.tsv", "rb").read() and len(table) > 100_000
    want = site_ref.site_file(table.decode(), _labels(chrs, pos), **ref_kw)
    assert open(tmp_path / "s.tsv").read() == want
    assert open(tmp_path / "s2.tsv").read() == want
    assert "\tNA\tNA\t" in want or all(int(ln.split("\t")[1]) > 0 for ln in want.splitlines()[1:])
    # signed values, and beside the other analyses
    r = run("--site_out", "s3.tsv", "--site_ld", "D", "--site_signed", "--decay_out", "b.tsv", "--prune_out", "k.txt")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "s3.tsv").read() == site_ref.site_file(table.decode(), _labels(chrs, pos), ld=("D",), abs_value=False)
    assert os.path.getsize(tmp_path / "b.tsv") > 0 and os.path.getsize(tmp_path / "k.txt") > 0
    # without --pos the sites are numbered from 1
    nopos = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "0", "--max_snp_dist", "20"]
    r = subprocess.run([*nopos, "--site_out", "s4.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = open(tmp_path / "s4.tsv").read().splitlines()
    assert len(rows) == n_sites + 1 and [ln.split("\t")[0] for ln in rows[1:4]] == ["1", "2", "3"]
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--site_out", "s5.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--site_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "s5.tsv")
