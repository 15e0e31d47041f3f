"""LD blocks on the device (ngsld_blocks, Engine.blocks / blocks_text, the binary's --blocks_* flags) against
tests/blocks_ref.py -- the restatement of LD_blocks.sh -- applied to the same engine's own TSV (run_text) and, where it is
built, to the reference program's table.  Every matrix file must be byte-identical."""
import ctypes as C
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


# ---- the blocks beside the other analyses' results: every store has one owner (results.h) ----
REFUSALS = {  # what each store's getters answer while it is empty
    "site_ld": "no ngsld_site_ld result (it goes with the next ngsld_plan or ngsld_set_*)",
    "clusters": "no ngsld_clusters result (it goes with the next ngsld_plan or ngsld_set_*)",
    "grid": "no ngsld_grid result (it goes with the next ngsld_plan or ngsld_set_*)",
    "scan": "no ngsld_scan result (it goes with the next ngsld_plan or ngsld_set_*)",
    "partners": "no ngsld_partners result (it goes with the next ngsld_plan or ngsld_set_*)",
    "blocks": "ngsld_blocks has not been called since the last plan or setting",
}


class Stores:
    """The smallest context in which every analysis leaves a result: 60 sites on two chromosomes, 8 individuals, a window of
    2 kb over gaps of up to 300 bp (every site has several pairs), the blocks' region a dozen sites of chr1.  fill() calls
    each analysis once through its entry point; read(name) copies a store out through its getters alone."""
    PLAN = dict(max_kb_dist=2, extend_out=False)

    def __init__(self):
        n, n_ind = 60, 8
        self.raw = synth.make_gl_numpy(n, n_ind, 23, depth=4.0)
        chrs, pos = synth.make_positions(n, 23, max_gap=300, n_chr=2)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
        self.region = ("chr1", int(pos[4]), int(pos[15]))
        self.eng = capi.Engine(0)
        try:
            self.eng.set_geno_raw(self.raw)
            self.eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
            assert self.eng.plan(**self.PLAN) > 60 * 3
            e = self.eng
            self.jobs = dict(decay=e._decay_job(ld=ALL4, bin_size=100), site_ld=e._site_ld_job(ld=ALL4, linked_min=0.1),
                             clusters=e._clusters_job(min_weight=0.1, min_size=1), grid=e._grid_job(self.labels, 1000, ld=ALL4),
                             scan=e._scan_job(500, ld=ALL4))
        except BaseException:
            self.eng.close()
            raise

    def fill(self, names=("decay", "site_ld", "clusters", "grid", "scan", "partners", "blocks")):
        for name in names:
            if name == "partners":
                self.eng.partners(3, min_weight=0.1)
            elif name == "blocks":
                assert self.eng.blocks(self.labels, *self.region, ld=ALL4)[2]["sites"] >= 10
            else:
                self.jobs[name].call()

    def read(self, name) -> dict:
        """The store's arrays as its getters return them now, by name; every getter must answer OK."""
        L, h = self.eng._L, self.eng._h
        if name == "partners":
            k, n, f = C.c_uint32(), C.c_uint64(), C.c_uint32()
            assert L.ngsld_partners_info(h, C.byref(k), C.byref(n), C.byref(f)) == capi.OK
            out = dict(info=np.array([k.value, n.value, f.value]), rows=np.zeros(n.value, dtype=np.uint64),
                       partner=np.zeros((n.value, k.value), dtype=np.uint32), value=np.zeros((n.value, k.value), dtype=np.int64))
            assert L.ngsld_partners_get(h, out["rows"].ctypes.data, out["partner"].ctypes.data, out["value"].ctypes.data) == capi.OK
            return out
        if name == "blocks":
            m = C.c_uint64()
            assert L.ngsld_blocks_sites(h, 0, None, C.byref(m)) == capi.OK
            m = m.value
            out = dict(sites=np.zeros(m, dtype=np.uint64))
            assert L.ngsld_blocks_sites(h, m, out["sites"].ctypes.data, None) == capi.OK
            for k, f in enumerate(ALL4):
                out[f], out[f"present_{f}"] = np.zeros((m, m)), np.zeros((m, m), dtype=np.uint8)
                assert L.ngsld_blocks_matrix(h, 4 + k, out[f].ctypes.data, out[f"present_{f}"].ctypes.data) == capi.OK
            return out
        out = {}
        for k, part in enumerate(self.jobs[name].read()[:-1]):  # (Engine's readers: the getters, each checked for OK)
            out.update({f"{k}_{key}": v for key, v in part.items()} if isinstance(part, dict) else {str(k): part})
        return out

    def refusal(self, name) -> str:
        """The named store's getters all answer ERR_INVALID; returns the message."""
        L, h = self.eng._L, self.eng._h
        n = C.c_uint64()
        codes = {"site_ld": lambda: [L.ngsld_site_ld_get(h, 7, None, None, None, None, None)],
                 "clusters": lambda: [L.ngsld_clusters_sites(h, None),
                                      L.ngsld_clusters_table(h, 1, 0, None, None, None, None, None, None, None, None, None, C.byref(n))],
                 "grid": lambda: [L.ngsld_grid_cells(h, 0, None, None, None, None, C.byref(n)), L.ngsld_grid_chromosomes(h, 0, None, C.byref(n)),
                                  L.ngsld_grid_get(h, 7, 0, None, None, None, None)],
                 "scan": lambda: [L.ngsld_scan_get(h, 7, None, None, None, None, None, None, None, None, None, None)],
                 "partners": lambda: [L.ngsld_partners_info(h, None, None, None), L.ngsld_partners_get(h, None, None, None)],
                 "blocks": lambda: [L.ngsld_blocks_sites(h, 0, None, C.byref(n)), L.ngsld_blocks_matrix(h, 7, None, None)]}[name]()
        assert codes and all(c == capi.ERR_INVALID for c in codes), (name, codes)
        return L.ngsld_last_error(h).decode()


def _same_bits(got: dict, want: dict, where):
    assert set(got) == set(want), where
    for key, w in want.items():
        g = got[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key)
        assert np.array_equal(np.frombuffer(g.tobytes(), np.uint8), np.frombuffer(w.tobytes(), np.uint8)), (where, key)


def test_a_blocks_call_wipes_no_other_result():
    s = Stores()
    try:
        others = ("site_ld", "clusters", "grid", "scan", "partners")
        s.fill(others)
        before = {name: s.read(name) for name in others}
        # every store holds something: sites with rows, clusters, cells, windows with rows, partners
        assert before["site_ld"]["0_n"].any() and len(before["clusters"]["1_id"]) > 0 and len(before["grid"]["0_n"]) > 0
        assert before["scan"]["0_n_lr"].any() and before["scan"]["0_n_ll"].any() and before["partners"]["rows"].any()
        s.fill(("blocks",))
        for name in others:
            _same_bits(s.read(name), before[name], name)
        # ... and in the other direction: the matrices outlive the next ngsld_site_ld
        blocks = s.read("blocks")
        assert len(blocks["sites"]) >= 10 and blocks["present_r2"].any()
        s.fill(("site_ld",))
        _same_bits(s.read("blocks"), blocks, "blocks")
        _same_bits(s.read("site_ld"), before["site_ld"], "site_ld again")
    finally:
        s.eng.close()


@pytest.mark.parametrize("how", ["plan", "set_geno_raw"])
def test_a_new_plan_or_matrix_empties_six_stores_and_keeps_the_decay_bins(how):
    s = Stores()
    try:
        s.fill()
        bins = s.read("decay")
        assert len(bins["0_n"]) > 3
        for name in REFUSALS:
            s.read(name)  # (filled: every getter answers OK)
        if how == "plan":
            s.eng.plan(**s.PLAN)
        else:
            s.eng.set_geno_raw(s.raw)
        for name, text in REFUSALS.items():
            assert s.refusal(name) == text, name
        _same_bits(s.read("decay"), bins, "decay")  # (indexed by distance, not by site: they stay until the next ngsld_decay)
    finally:
        s.eng.close()
