"""LD blocks on the device (ngsld_blocks, Engine.blocks / blocks_text, the binary's --blocks_* flags) against
tests/blocks_ref.py -- the restatement of LD_blocks.sh -- applied to the same engine's own TSV (run_text) and, where it is
built, to the reference program's table.  Every matrix file must be byte-identical."""
import os
import subprocess

import numpy as np
import pytest

import blocks_ref
from ngsld_amd import capi, shard, synth
from util import have_ref_program

pytestmark = pytest.mark.gpu

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
KNOBS = ("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", "NGSLD_TEST_BLOCKS_HOST_ROWS", "NGSLD_TEST_BLOCKS_TEXT_ROWS")


def _positions(kind: str, n: int, seed: int):
    if kind == "reappear":  # chr1, chr2, chr1 again at lower positions: file order is not position order
        k = n // 3
        _, p = synth.make_positions(n, seed, max_gap=300)
        chrs = ["chr1"] * k + ["chr2"] * k + ["chr1"] * (n - 2 * k)
        pos = np.concatenate([p[:k] + 200_000, p[:k], p[: n - 2 * k]])
        return chrs, pos
    return synth.make_positions(n, seed, max_gap=300, n_chr=2 if kind in ("rnd_sample", "allpairs") else 1)


def _raw(kind: str, n: int, n_ind: int, seed: int):
    if kind == "hard":
        return np.eye(3)[synth.make_gl_numpy(n, n_ind, seed, depth=8.0).argmax(2)]
    return synth.make_gl_numpy(n, n_ind, seed, depth=4.0, mono_frac=0.2 if kind == "uncalled" else 0.0)


# kind: (n_sites, n_ind, plan kw)
KINDS = {
    "lkl": (400, 32, dict(max_kb_dist=10)),
    "uncalled": (400, 64, dict(max_kb_dist=10)),
    "hard": (400, 16, dict(max_kb_dist=10)),
    "rnd_sample": (400, 32, dict(max_kb_dist=15, rnd_sample=0.6, seed=7)),
    "snp_window": (400, 32, dict(max_snp_dist=25)),
    "allpairs": (240, 32, dict(max_kb_dist=0)),
    "reappear": (300, 32, dict(max_kb_dist=0)),
}


class Run:
    """One engine with its plan and its own TSV."""

    def __init__(self, kind: str):
        n, n_ind, plan_kw = KINDS[kind]
        seed = 300 + n + n_ind + len(kind)
        self.chrs, self.pos = _positions(kind, n, seed)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(self.chrs, self.pos)]
        self.eng = capi.Engine(0)
        self.eng.set_geno_raw(_raw(kind, n, n_ind, seed))
        self.eng.set_pos_dist(shard.pos_dist_from_positions(self.chrs, self.pos))
        self.eng.plan(extend_out=False, **plan_kw)
        self.eng.set_text_output(self.labels)
        text, fallbacks = self.eng.run_text()
        assert fallbacks == 0
        self.tsv = text.decode()
        self.row_off, _ = self.eng.plan_rows()

    def member_pairs(self, chr, start, end) -> int:
        m = np.array([c == chr and start <= p <= end for c, p in zip(self.chrs, self.pos)])
        return int(np.diff(self.row_off)[m].sum())

    def regions(self):
        """Strictly inside chr1 (windows cross both edges), all of chr1, one pair."""
        p1 = np.sort(np.array([p for c, p in zip(self.chrs, self.pos) if c == "chr1"]))
        out = {"inside": (int(p1[len(p1) // 4]) + 1, int(p1[len(p1) * 3 // 5])), "whole": (0, int(p1[-1]) + 1)}
        for ln in self.tsv.split("\n")[:200]:
            f = ln.split("\t")
            if len(f) > 2 and f[0].startswith("chr1:") and f[1].startswith("chr1:"):
                a, b = sorted((int(f[0][5:]), int(f[1][5:])))
                if a < b and sum(a <= p <= b for p in p1) == 2:
                    out["pair"] = (a, b)
                    break
        return out


@pytest.fixture(scope="module", params=list(KINDS))
def run(request):
    r = Run(request.param)
    yield r
    r.eng.close()


def check(run, chr, start, end, ld, tsv=None):
    """Engine.blocks against blocks_ref on the TSV: the files byte for byte, the sites, the counts; returns the stats."""
    sites, mats, st = run.eng.blocks(run.labels, chr, start, end, ld=ld)
    want_sites, files, info = blocks_ref.blocks(run.tsv if tsv is None else tsv, chr, start, end, ld=ld)
    assert [run.labels[s] for s in sites] == want_sites
    assert st["sites"] == info["sites"] and st["pairs_in_region"] == info["pairs_in_region"]
    assert st["pairs"] == run.member_pairs(chr, start, end)
    assert st["cells_na"] == st["sites"] ** 2 - st["pairs_in_region"]
    for f in ld:
        got = run.eng.blocks_text(f).decode()
        assert got == files[f], (f, _first_diff(got, files[f]))
        values, present = mats[f]
        cells = [ln.split("\t")[1:] for ln in files[f].split("\n")[1:-1]]
        assert np.array_equal(present.astype(bool), np.array(cells, dtype=object).reshape(present.shape) != "NA")
        assert np.isnan(values[present == 0]).all()
    return st


def _first_diff(a: str, b: str):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, a[max(0, k - 60): k + 60], b[max(0, k - 60): k + 60]


@pytest.mark.parametrize("region", ["inside", "whole", "pair"])
def test_blocks_equal_the_script_on_own_tsv(run, region, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    regions = run.regions()
    if region not in regions:
        pytest.skip("no adjacent pair of chr1 among the first rows")
    start, end = regions[region]
    st = check(run, "chr1", start, end, ALL4 if region != "inside" else ("r2", "Dp"))
    assert st["sites"] > 0 and (st["pairs_in_region"] == 1) == (region == "pair")
    print(f"{region}: {st['members']} members, {st['sites']} sites, {st['pairs_in_region']} of {st['pairs']} pairs; "
          f"pairs {st['pairs_ms']:.1f} ms, scatter {st['scatter_ms']:.2f} ms")


def test_knobs_give_the_same_bytes(monkeypatch):
    r = Run("uncalled")
    try:
        start, end = r.regions()["inside"]
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        st0 = check(r, "chr1", start, end, ALL4)
        base = {f: r.eng.blocks_text(f) for f in ALL4}
        assert st0["chunks"] == 1 and st0["sites"] > 20
        monkeypatch.setenv("NGSLD_TEST_BLOCKS_CHUNK_PAIRS", "300")
        st1 = check(r, "chr1", start, end, ALL4)
        assert st1["chunks"] > 5 and st1["pairs"] == st0["pairs"]
        monkeypatch.setenv("NGSLD_TEST_BLOCKS_HOST_ROWS", "1")
        info = {}
        assert r.eng.blocks_text("Dp", info) == base["Dp"] and info["host_rows"] == st0["sites"]
        monkeypatch.delenv("NGSLD_TEST_BLOCKS_HOST_ROWS")
        monkeypatch.setenv("NGSLD_TEST_BLOCKS_TEXT_ROWS", "3")
        for f in ALL4:
            info = {}
            assert r.eng.blocks_text(f, info) == base[f] and info["host_rows"] == 0
            assert info["pieces"] >= 1 + st0["sites"] // 3
    finally:
        r.eng.close()


def test_matrix_values_are_the_records_bits_and_two_calls_agree():
    r = Run("hard")
    try:
        start, end = r.regions()["inside"]
        sites, mats, st = r.eng.blocks(r.labels, "chr1", start, end, ld=ALL4)
        text = {f: r.eng.blocks_text(f) for f in ALL4}
        sites2, mats2, _ = r.eng.blocks(r.labels, "chr1", start, end, ld=ALL4)
        assert np.array_equal(sites, sites2)
        for f in ALL4:
            assert r.eng.blocks_text(f) == text[f]
            assert mats[f][0].tobytes() == mats2[f][0].tobytes() and np.array_equal(mats[f][1], mats2[f][1])
        r.eng.set_text_output(None, False)
        s1, s2, std, _ = r.eng.run()
    finally:
        r.eng.close()
    at = {int(s): k for k, s in enumerate(sites)}
    seen = 0
    for i in range(len(s1)):
        a, b = at.get(int(s1[i])), at.get(int(s2[i]))
        if a is None or b is None:
            continue
        seen += 1
        for f in ALL4:
            assert mats[f][1][a, b] == 1
            got, rec = mats[f][0][a, b], float(std[f][i])
            assert got == rec or (np.isnan(got) and np.isnan(rec)) or abs(got - rec) < 1e-12, (f, i, got, rec)
    assert seen == st["pairs_in_region"] > 0
    for f in ALL4:  # the values are the doubles the cells print: the host's "%f" of each is the cell's text
        cells = [ln.split("\t")[1:] for ln in text[f].decode().split("\n")[1:-1]]
        for a, b in zip(*np.nonzero(mats[f][1])):
            assert capi.format_double(float(mats[f][0][a, b])) == cells[a][b], (f, a, b)


def test_extra_pos_column_gives_the_same_matrices():
    r = Run("lkl")
    try:
        start, end = r.regions()["inside"]
        sites, _, _ = r.eng.blocks(r.labels, "chr1", start, end)
        text = {f: r.eng.blocks_text(f) for f in ("r2", "Dp")}
        extra = [f"{l}\tsnp{k}" for k, l in enumerate(r.labels)]
        sites2, _, _ = r.eng.blocks(extra, "chr1", start, end)
        assert np.array_equal(sites, sites2)
        for f in ("r2", "Dp"):
            assert r.eng.blocks_text(f) == text[f]
    finally:
        r.eng.close()


def test_refusals_and_an_empty_region():
    r = Run("reappear")
    try:
        with pytest.raises(capi.NgsldError) as e:
            r.eng.blocks(None, "chr1", 1, 10)
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(capi.NgsldError) as e:
            r.eng.blocks(["(null)"] * len(r.labels), "chr1", 1, 10)
        assert e.value.code == capi.ERR_INVALID
        bad = list(r.labels)
        bad[5] = "chr1:12x"
        sites, _, _ = r.eng.blocks(bad, "chr2", 0, 10 ** 9)  # (a bad position of another chromosome is no concern)
        assert len(sites) > 0
        with pytest.raises(capi.NgsldError) as e:
            r.eng.blocks(bad, "chr1", 0, 10 ** 9)
        assert e.value.code == capi.ERR_UNSUPPORTED and "chr1:12x" in e.value.msg
        dup = list(r.labels)
        dup[-1] = dup[0]                                   # chr1 reappears at a position it had
        with pytest.raises(capi.NgsldError) as e:
            r.eng.blocks(dup, "chr1", 0, 10 ** 9)
        assert e.value.code == capi.ERR_UNSUPPORTED and dup[0] in e.value.msg
        sites, mats, st = r.eng.blocks(r.labels, "chr3", 0, 10 ** 9)
        assert len(sites) == 0 and st["sites"] == 0 and r.eng.blocks_text("r2") == b"\n"
    finally:
        r.eng.close()


def test_too_many_members_are_refused():
    n = 33_000
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(synth.make_gl_numpy(n, 4, 5, depth=4.0))
        eng.set_pos_dist(np.ones(n))
        eng.plan(max_snp_dist=1, extend_out=False)
        with pytest.raises(capi.NgsldError) as e:
            eng.blocks([f"c:{k + 1}" for k in range(n)], "c", 1, n)
        assert e.value.code == capi.ERR_UNSUPPORTED and "33000 region members" in e.value.msg
    finally:
        eng.close()


def test_binary_blocks_out(tmp_path):
    n_sites, n_ind = 400, 32
    raw = synth.make_gl_numpy(n_sites, n_ind, 97, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 97, max_gap=300, n_chr=2)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    start, end = int(pos[40]), int(pos[150])
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "10",
            "--blocks_chr", "chr1", "--blocks_start", str(start), "--blocks_end", str(end)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    r = subprocess.run([*base, "--out", "t.tsv", "--blocks_out", "P", "--blocks_ld", "r2,Dp,D"], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    sites, files, info = blocks_ref.blocks(open(tmp_path / "t.tsv").read(), "chr1", start, end, ld=("r2", "Dp", "D"))
    for f in ("r2", "Dp", "D"):
        assert open(tmp_path / f"P.{f}.tsv").read() == files[f], f
    assert not os.path.exists(tmp_path / "P.r2_ExpG.tsv")
    assert f"==> LD blocks: {info['sites']} sites, {info['pairs_in_region']} pairs in region" in r.stderr
    r = subprocess.run([*base, "--blocks_out", "Q"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == ""                                           # no TSV without --out
    assert open(tmp_path / "Q.r2.tsv").read() == files["r2"] and open(tmp_path / "Q.Dp.tsv").read() == files["Dp"]
    assert sorted(os.listdir(tmp_path)) == ["P.D.tsv", "P.Dp.tsv", "P.r2.tsv", "Q.Dp.tsv", "Q.r2.tsv", "g.bin", "p.pos", "t.tsv"]
    r = subprocess.run([*base[:-6], "--blocks_chr", "chr9", "--blocks_start", "1", "--blocks_end", "9", "--blocks_out", "R"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300, env=env)
    assert r.returncode == 255 and "no SNPs found in region." in r.stderr


@pytest.mark.skipif(not have_ref_program(), reason="oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")
@pytest.mark.parametrize("name", ["called_n8", "text_n8_missing"])
def test_blocks_of_the_reference_table(name, tmp_path):
    """Tie-heavy called genotypes: -0.000000 and odd / 128 ties in the cells, against the reference program's own table."""
    from test_gpu_ties import Case, _ref_table
    case = Case(name, str(tmp_path))
    want_text = _ref_table(case, False, str(tmp_path))
    p1 = np.sort(np.asarray(case.pos))
    start, end = int(p1[30]), int(p1[220])
    eng = case.engine()
    try:
        eng.plan(extend_out=False)

        class R:
            pass
        r = R()
        r.eng, r.labels, r.tsv = eng, case.labels, want_text
        r.chrs, r.pos = case.chrs, case.pos
        r.row_off, _ = eng.plan_rows()
        r.member_pairs = lambda c, s, e: Run.member_pairs(r, c, s, e)
        st = check(r, case.chrs[0], start, end, ALL4)
    finally:
        eng.close()
    _, files, _ = blocks_ref.blocks(want_text, case.chrs[0], start, end, ld=("D",))
    assert "-0.000000" in files["D"] or "\t0.000000" in files["D"]
    print(f"{name}: {st['sites']} sites, {st['pairs_in_region']} pairs identical to the script on the reference table")
