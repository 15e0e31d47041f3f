"""LD decay on the device (ngsld_decay, Engine.decay, the binary's --decay_* flags) against tests/decay_ref.py -- the
restatement of fit_LDdecay.R's binning -- applied to the same engine's own TSV (run_text).  Counts must be equal and every
mean must be the double nearest to the exact mean of the printed decimals."""
import os
import subprocess

import numpy as np
import pytest

import decay_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _tsv(eng, chrs, pos):
    eng.set_text_output([f"{c}:{int(p)}" for c, p in zip(chrs, pos)])
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _same(bins, want, ld):
    chosen = [f for f in decay_ref.FIELDS if f in ld]
    assert len(bins["dist"]) == len(want), (len(bins["dist"]), len(want))
    assert [float(x) for x in bins["dist"]] == [w[0] for w in want]
    assert [int(x) for x in bins["n"]] == [w[1] for w in want]
    for f in chosen:
        got = bins[f]
        exp = np.array([float(w[2][f]) for w in want])
        bad = np.nonzero(got.view(np.int64) != exp.view(np.int64))[0]
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _case(raw, chrs, pos, plan_kw, decay_kw, geno_kw=None):
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, chrs, pos)
        bins, stats = eng.decay(**decay_kw)
    finally:
        eng.close()
    ld = decay_kw.get("ld", ("r2",))
    ref_kw = {k: v for k, v in decay_kw.items()}
    want = decay_ref.decay_bins(text, **ref_kw)
    _same(bins, want, ld)
    assert stats["bins"] == len(want) and stats["pairs_counted"] == sum(w[1] for w in want)
    return bins, stats, want


# extend_out everywhere: the reference restatement applies the maf filter where the TSV has maf1 / maf2, as the script does
WIN = dict(max_kb_dist=20, extend_out=True)
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, decay kw, geno kw)
    "n8_window": (500, 8, {}, 1, WIN, {}, None),
    "n64_window": (500, 64, {}, 1, WIN, {}, None),
    "n500_window": (400, 500, {}, 1, WIN, {}, None),
    "allpairs_two_chr": (300, 64, {}, 2, dict(extend_out=True), {}, None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=30, min_maf=0.1, rnd_sample=0.6, seed=7, extend_out=True), {}, None),
    "decay_min_maf": (500, 64, {}, 1, WIN, dict(min_maf=0.2), None),
    "all_four": (400, 64, {}, 1, WIN, dict(ld=ALL4), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, dict(ld=ALL4), None),
    "uncalled_mono_r2": (500, 64, dict(mono_frac=0.2), 1, WIN, {}, None),
    "call_geno": (500, 64, {}, 1, WIN, dict(ld=("r2", "Dp")), dict(call_geno=(0.1, 0.9))),
    "bin_2": (300, 64, {}, 1, WIN, dict(bin_size=2), None),
    "bin_62.5": (400, 64, {}, 1, WIN, dict(bin_size=62.5, ld=("D", "r2")), None),
    "bin_1000": (400, 64, {}, 1, WIN, dict(bin_size=1000), None),
    "bin_250_kb_limit": (400, 64, {}, 1, WIN, dict(bin_size=250, max_kb_dist=7.5), None),
    # bin sizes that are not dyadic: k * B is rounded, bin_of's corrections and the %.15g break labels come into play
    "bin_33.3": (400, 64, {}, 1, WIN, dict(bin_size=33.3, ld=ALL4), None),
    "bin_1.1": (300, 64, {}, 1, dict(max_kb_dist=3, extend_out=True), dict(bin_size=1.1), None),
    "bin_7.3": (400, 8, {}, 1, WIN, dict(bin_size=7.3, ld=("D", "r2")), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_decay_equals_script_on_own_tsv(name):
    n_sites, n_ind, skw, n_chr, plan_kw, decay_kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 500 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 37, max_gap=300, n_chr=n_chr)
    _, stats, want = _case(raw, chrs, pos, plan_kw, decay_kw, geno_kw)
    assert len(want) > 0 and stats["pairs_counted"] > 0


def test_limit_on_a_present_dist():
    """max_kb_dist * 1000 equal to a dist the TSV holds: the script's filter is strict, those rows are out."""
    raw = synth.make_gl_numpy(300, 64, 61, depth=4.0)
    chrs, pos = synth.make_positions(300, 61, max_gap=300)
    d = next(float(pos[k] - pos[0]) for k in range(60, 300) if (float(pos[k] - pos[0]) / 1000) * 1000 == float(pos[k] - pos[0]))
    _, _, want = _case(raw, chrs, pos, dict(extend_out=True), dict(max_kb_dist=d / 1000))
    assert max(w[0] for w in want) < d
    eng = _engine(raw, chrs, pos, dict(extend_out=True))
    try:
        text = _tsv(eng, chrs, pos)
    finally:
        eng.close()
    assert f"\t{int(d)}\t" in text  # (the limit is a dist of the table)


@pytest.mark.parametrize("bin_size", [33.3, 7.3, 1.1])
def test_dist_on_an_inexact_break(bin_size):
    """Sites at every position 1..400: every integer dist is in the table, among them breaks k * B that round to an integer
    (10 * 33.3 == 333.0), where d / B lands a hair above k and only the right-closed rule puts the row in bin k - 1."""
    n = 400
    raw = synth.make_gl_numpy(n, 16, 23, depth=4.0)
    chrs, pos = ["chr1"] * n, np.arange(1, n + 1)
    on_break = [k * bin_size for k in range(1, int(n / bin_size) + 1) if k * bin_size == int(k * bin_size)]
    assert on_break
    _, _, want = _case(raw, chrs, pos, dict(extend_out=True, max_kb_dist=0), dict(bin_size=bin_size, ld=ALL4))
    labels = [w[0] for w in want]
    assert all(float(f"{b:.15g}") in labels for b in on_break if b < n - 1)
    print(f"bin {bin_size}: {len(want)} bins, dists on the breaks {on_break[:4]}")


def _knob_case(monkeypatch, env):
    for k in ("NGSLD_TEST_DECAY_LDS_BYTES", "NGSLD_TEST_DECAY_CHUNK_PAIRS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    raw = synth.make_gl_numpy(600, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(600, 71, max_gap=300)
    return _case(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True), dict(ld=ALL4))


def test_lds_global_and_small_chunks_give_the_same_bins(monkeypatch):
    b0, s0, _ = _knob_case(monkeypatch, {})
    assert s0["lds"] == 1 and s0["chunks"] == 1
    b1, s1, _ = _knob_case(monkeypatch, {"NGSLD_TEST_DECAY_LDS_BYTES": "0"})
    assert s1["lds"] == 0
    b2, s2, _ = _knob_case(monkeypatch, {"NGSLD_TEST_DECAY_CHUNK_PAIRS": "3000"})
    assert s2["chunks"] > 5
    b3, s3, _ = _knob_case(monkeypatch, {"NGSLD_TEST_DECAY_CHUNK_PAIRS": "3000", "NGSLD_TEST_DECAY_LDS_BYTES": "0"})
    assert s3["lds"] == 0 and s3["chunks"] == s2["chunks"]
    for b in (b1, b2, b3):
        assert b.keys() == b0.keys()
        for k in b0:
            assert b[k].tobytes() == b0[k].tobytes(), k


def test_all_pairs_many_bins_take_the_global_path():
    """All pairs with no window over one chromosome at bin size 2: tens of thousands of bins, beyond the LDS budget."""
    raw = synth.make_gl_numpy(400, 32, 83, depth=4.0)
    chrs, pos = synth.make_positions(400, 83, max_gap=300)
    _, stats, want = _case(raw, chrs, pos, dict(extend_out=True), dict(bin_size=2))
    assert stats["lds"] == 0 and stats["bin_slots"] > 10_000 and len(want) > 1000


def test_two_calls_give_the_same_bits():
    raw = synth.make_gl_numpy(500, 64, 91, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 91, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        a, sa = eng.decay(ld=ALL4)
        b, sb = eng.decay(ld=ALL4)
    finally:
        eng.close()
    assert sa["bins"] == sb["bins"] > 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _read_tab(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:-1]]


def test_cli_decay_out_and_fit(tmp_path):
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
    dk = ["--decay_ld", "Dp,r2", "--decay_bin_size", "500", "--decay_min_maf", "0.05"]
    r = run("--out", "t.tsv", "--decay_out", "b.tsv", "--decay_fit", "f.tsv", *dk)
    assert r.returncode == 0, r.stderr[-2000:]
    want = decay_ref.decay_bins(open(tmp_path / "t.tsv").read(), ld=("Dp", "r2"), bin_size=500, min_maf=0.05)
    head, rows = _read_tab(tmp_path / "b.tsv")
    assert head == ["dist", "n", "Dp", "r2"]
    assert len(rows) == len(want) > 0
    for row, w in zip(rows, want):
        assert float(row[0]) == w[0] and int(row[1]) == w[1]
        assert float(row[2]) == float(w[2]["Dp"]) and float(row[3]) == float(w[2]["r2"])
    dist = np.array([float(r_[0]) for r_ in rows])
    fh, frows = _read_tab(tmp_path / "f.tsv")
    assert fh == ["LD", "DecayRate", "LDmax", "LDmin", "SSE", "n_bins"]
    assert [f[0] for f in frows] == ["Dp", "r2"]
    for f, col in zip(frows, (2, 3)):
        fit = capi.decay_fit(dist, np.array([float(r_[col]) for r_ in rows]), f[0])
        assert [float(x) for x in f[1:5]] == [fit["rate"], fit["ld_max"], fit["ld_min"], fit["sse"]] and int(f[5]) == len(rows)
    # --decay_out alone: the same bins, no TSV (not even on standard output)
    r = run("--decay_out", "b2.tsv", *dk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == ""
    assert open(tmp_path / "b2.tsv").read() == open(tmp_path / "b.tsv").read()
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--decay_out", "b3.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--decay_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "b3.tsv")
