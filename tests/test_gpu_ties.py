"""GPU: input whose LD values sit exactly on a rounding tie of "%f", end to end.

x * 10^6 ends in exactly .5 only for x = odd / 128, and called genotypes of small cohorts give D values like that by the
thousand (n_ind 8: some 1,500 of 44,850 pairs; n_ind 64: hundreds of haplotype frequencies).  There a difference of one ulp,
which the 1e-9 bar of the record checks lets through, turns the printed digit -- in the TSV, in LD pruning's edge labels and in
LD decay's sums.  So on such input: (a) the records of every tie are the oracle's bits, on both kernel paths; (b) the binary's
table is the reference program's, byte for byte; (c) LD decay's bins and (d) LD pruning's sets equal what the scripts' rules
make of the REFERENCE program's table (not the engine's own, which a wrong device value would bend the same way).  Every case
first asserts that it holds the ties it is about."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import decay_ref
import prune_ref
from ngsld_amd import capi, shard, synth
from oracle import orc
from printed_values import is_tie
from test_gpu_decay import _same as same_bins
from test_gpu_vs_ref_program import same_tsv
from util import check_records, have_ref_program, run_ref_program

pytestmark = pytest.mark.gpu

N_SITES = 300


def _called(n_ind: int) -> np.ndarray:
    return np.eye(3)[synth.make_gl_numpy(N_SITES, n_ind, 7 + n_ind, depth=8.0).argmax(2)]


# name: (n_ind, input kind, minimum exact ties of D, of hap in the oracle's records)
CASES = {
    "called_n8": (8, "bin", 1000, 0),
    "called_n16": (16, "bin", 150, 0),
    "called_n64": (64, "bin", 0, 300),
    "text_n8_missing": (8, "text", 500, 50),
    "call_geno_n8": (8, "call_geno", 1000, 0),
}
CALL = (0.1, 0.6)


class Case:
    """The input of one case as files (for the two programs) and as the engine takes it, and the oracle's records."""

    def __init__(self, name: str, d: str):
        n_ind, kind, self.min_d, self.min_hap = CASES[name]
        self.n_ind, self.kind = n_ind, kind
        self.chrs, self.pos = synth.make_positions(N_SITES, 40 + n_ind, max_gap=300)
        self.pd = shard.pos_dist_from_positions(self.chrs, self.pos)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(self.chrs, self.pos)]
        self.ppath = os.path.join(d, "in.pos")
        synth.write_pos(self.ppath, self.chrs, self.pos)
        self.flags = ["--n_ind", str(n_ind), "--n_sites", str(N_SITES), "--verbose", "0", "--pos", self.ppath]
        self.call = None
        if kind == "text":
            g = _called(n_ind).argmax(2).astype(float)
            g[np.random.default_rng(n_ind).random(g.shape) < 0.05] = -1.0    # no call
            self.gpath = os.path.join(d, "in.geno.gz")
            with gzip.open(self.gpath, "wt") as fh:
                fh.write("".join("\t".join(str(int(x)) for x in row) + "\n" for row in g))
            gl = np.empty((N_SITES, n_ind, 3))
            err = C.create_string_buffer(256)
            rc = orc.lib().orc_read_geno_text(self.gpath.encode(), 0, 0, n_ind, N_SITES, orc.dp(gl), err, 256)
            assert rc == 0, err.value
            self.oracle = orc.Oracle(gl, self.pd, already_normalised_log=True, n_threads=8)
            self.flags += ["--geno", self.gpath]
        else:
            if kind == "call_geno":
                self.raw = synth.make_gl_numpy(N_SITES, n_ind, 7 + n_ind, depth=8.0)
                self.call = CALL
                self.flags += ["--probs", "--call_geno", "--N_thresh", repr(CALL[0]), "--call_thresh", repr(CALL[1])]
            else:
                self.raw = _called(n_ind)
            self.gpath = os.path.join(d, "in.glf")
            self.raw.tofile(self.gpath)
            self.oracle = orc.Oracle(self.raw, self.pd, n_threads=8, call_geno=self.call)
            self.flags += ["--geno", self.gpath]
        self.rec = self.oracle.run()
        self.d_ties = is_tie(self.rec["D"])
        self.hap_ties = is_tie(self.rec["hap"])

    def engine(self) -> capi.Engine:
        eng = capi.Engine(0)
        if self.kind == "text":
            raw, is_log = capi.read_geno_text(self.gpath, False, False, self.n_ind, N_SITES)
            eng.set_geno_raw(raw, log_scale=is_log, text=True)
        else:
            eng.set_geno_raw(self.raw, call_geno=self.call)
        eng.set_pos_dist(self.pd)
        return eng


@pytest.fixture(scope="module", params=list(CASES))
def case(request, tmp_path_factory):
    c = Case(request.param, str(tmp_path_factory.mktemp(request.param)))
    n_d, n_h = int(c.d_ties.sum()), int(c.hap_ties.sum())
    print(f"\n{request.param}: {len(c.rec)} pairs, {n_d} D and {n_h} hap values exactly on a tie")
    assert n_d >= c.min_d and n_h >= c.min_hap, (n_d, n_h)
    return c


@pytest.mark.parametrize("path", ["hard", "generic"])
def test_tie_records_are_the_oracles_bits(case, path, monkeypatch):
    """(a) every record within 1e-9 of the oracle, and where the oracle's D or hap is a tie, the same bits."""
    if path == "generic":
        monkeypatch.setenv("NGSLD_TEST_HARD_KERNEL", "0")
    else:
        monkeypatch.delenv("NGSLD_TEST_HARD_KERNEL", raising=False)
    eng = case.engine()
    try:
        if case.kind != "call_geno":   # (hardened likelihoods with calls below N_thresh stay on the per-individual kernels)
            assert (eng.pair_kernel() == "hard") == (path == "hard")
        assert eng.plan(extend_out=True) == len(case.rec)
        s1, s2, std, ext = eng.run()
    finally:
        eng.close()
    assert np.array_equal(s1, case.rec["s1"]) and np.array_equal(s2, case.rec["s2"])
    check_records(std, ext, case.rec)
    dt, ht = case.d_ties, case.hap_ties
    bad = np.flatnonzero(std["D"][dt].view(np.uint64) != case.rec["D"][dt].view(np.uint64))
    assert len(bad) == 0, (f"{len(bad)} of {dt.sum()} tie D values differ from the oracle's bits: got "
                           f"{std['D'][dt][bad[:3]].tolist()} want {case.rec['D'][dt][bad[:3]].tolist()}")
    bad = np.flatnonzero(ext["hap"][ht].view(np.uint64) != case.rec["hap"][ht].view(np.uint64))
    assert len(bad) == 0, f"{len(bad)} of {ht.sum()} tie hap values differ from the oracle's bits"
    # the float chi2 the extended columns print, from these hap values, against the oracle's (ngsLD.cpp:328-333)
    got_chi2 = np.array(["%f" % v for v in _chi2(ext["hap"])])
    want_chi2 = np.array(["%f" % v for v in case.rec["chi2"].astype(np.float64)])
    bad = np.flatnonzero(got_chi2 != want_chi2)
    assert len(bad) == 0, f"{len(bad)} chi2 print differently, first {got_chi2[bad[:3]]} against {want_chi2[bad[:3]]}"
    print(f"{path}: {int(dt.sum())} tie D and {int(ht.sum())} tie hap values bit-identical, every chi2 printed the same")


def _chi2(hap: np.ndarray) -> np.ndarray:
    """ngsLD.cpp:328-333 over rows of hap[4]: float frequencies and products, each step summed in double, stored in float."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        fa, fb = (hap[:, 0] + hap[:, 1]).astype(f32), (hap[:, 0] + hap[:, 2]).astype(f32)
        exp_hap = [fa * fb, fa * (f32(1) - fb), (f32(1) - fa) * fb, (f32(1) - fa) * (f32(1) - fb)]
        chi2 = np.zeros(len(hap), dtype=f32)
        for i in range(4):
            e = exp_hap[i].astype(np.float64)
            d = hap[:, i] - e
            chi2 = (chi2.astype(np.float64) + d * d / e).astype(f32)
    return chi2.astype(np.float64)


def _ref_table(case, extend: bool, d: str) -> str:
    out = os.path.join(d, f"ref_{int(extend)}.tsv")
    if not os.path.exists(out):
        r = run_ref_program(case.rec, N_SITES, case.flags + (["--extend_out"] if extend else []), out, d, threads=4)
        assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


needs_ref = pytest.mark.skipif(not have_ref_program(), reason="oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")


@needs_ref
@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("text", ["device", "host"])
def test_table_is_the_reference_programs(case, extend, text, tmp_path):
    """(b) the binary's table against the reference program's, sorted bodies identical, rows made on the device and on the
    host formatter (NGSLD_HOST_TEXT=1).  (The extended table of the text file once differed in one chi2: a hap sum exactly on a
    float midpoint that the kernel's hap, a few ulp off, rounded the other way.)"""
    d = os.path.dirname(case.ppath)
    want = _ref_table(case, extend, d)
    out = str(tmp_path / "hip.tsv")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_")}
    if text == "host":
        env["NGSLD_HOST_TEXT"] = "1"
    flags = case.flags + (["--extend_out"] if extend else [])
    h = subprocess.run([capi.CLI_PATH, *flags, "--n_threads", "2", "--out", out], capture_output=True, text=True, timeout=300,
                       env=env)
    assert h.returncode == 0, h.stderr[-2000:]
    got = open(out).read()
    assert same_tsv(got, want) is None, same_tsv(got, want)
    print(f"table ({text} text, extend_out {extend}): {len(want.splitlines()) - 1} rows identical, "
          f"{int(case.d_ties.sum())} with a tie D")


@needs_ref
@pytest.mark.parametrize("bin_size", [250, 33.3])
def test_decay_bins_of_the_reference_table(case, bin_size):
    """(c) LD decay on the device against fit_LDdecay.R's binning of the reference program's table, bit for bit; min_maf is
    a frequency the table prints (k / (2 n_ind) for called genotypes), so the maf filter's >= meets equality."""
    if case.kind == "call_geno" or case.n_ind > 16:
        pytest.skip("decay and pruning run on the called cohorts of 8 and 16 and the text file")
    want_text = _ref_table(case, True, os.path.dirname(case.ppath))
    min_maf = 1.0 / case.n_ind
    assert f"\t{min_maf:f}\t" in want_text
    ld = ("r2_ExpG", "D", "Dp", "r2")
    eng = case.engine()
    try:
        eng.plan(extend_out=True)
        bins, stats = eng.decay(ld=ld, bin_size=bin_size, min_maf=min_maf)
    finally:
        eng.close()
    want = decay_ref.decay_bins(want_text, ld=ld, bin_size=bin_size, min_maf=min_maf)
    same_bins(bins, want, ld)
    assert stats["pairs_counted"] == sum(w[1] for w in want) > 0
    print(f"decay bin {bin_size}: {len(want)} bins, {stats['pairs_counted']} rows equal to the script on the reference table; "
          f"pairs with their replay {stats['pairs_ms']:.1f} ms, bins {stats['bin_ms']:.2f} ms, call {stats['total_ms']:.1f} ms")


@needs_ref
def test_prune_sets_of_the_reference_table(case):
    """(d) LD pruning on D (field 5) against prune_graph.pl's rule on the reference program's table: weight types a and e,
    precision 6 (where the two roundings of a tie give different labels) and 4, min_weight a printed weight of a tie."""
    if case.kind == "call_geno" or case.n_ind > 16:
        pytest.skip("decay and pruning run on the called cohorts of 8 and 16 and the text file")
    want_text = _ref_table(case, True, os.path.dirname(case.ppath))
    vals, counts = np.unique(np.abs(case.rec["D"][case.d_ties]), return_counts=True)
    mw = float(f"{vals[np.argmax(counts)]:f}")        # the commonest tie |D|, as printed
    eng = case.engine()
    checked = 0
    try:
        eng.plan(extend_out=False)
        for wtype in "ae":
            for prec in (6, 4):
                for min_weight in (0.0, mw):
                    state, stats = eng.prune(case.labels, field=5, weight_type=wtype, precision=prec, min_weight=min_weight)
                    kept, excl = prune_ref.prune_tsv(want_text, field=5, weight_type=wtype, precision=prec,
                                                     min_weight=min_weight)
                    got_kept = {case.labels[s] for s in np.nonzero(state == 1)[0]}
                    got_excl = {case.labels[s] for s in np.nonzero(state == 2)[0]}
                    assert got_kept == kept and got_excl == excl, (wtype, prec, min_weight, len(got_kept ^ kept))
                    assert stats["edges"] > 0
                    checked += 1
                    pairs_ms = stats["pairs_ms"]
    finally:
        eng.close()
    print(f"prune: {checked} settings equal to the script on the reference table (min_weight {mw} a printed tie weight); "
          f"pairs with their replay {pairs_ms:.1f} ms")
