"""GPU: input whose LD values sit exactly on a rounding tie of "%f", end to end.

x * 10^6 ends in exactly .5 only for x = odd / 128, and called genotypes of small cohorts give D values like that by the
thousand (n_ind 8: some 1,500 of 44,850 pairs; n_ind 64: hundreds of haplotype frequencies).  There a difference of one ulp,
which the 1e-9 bar of the record checks lets through, turns the printed digit -- in the TSV, in LD pruning's edge labels and in
LD decay's sums.  So on such input: (a) the records of every tie are the oracle's bits, on both kernel paths; (b) the binary's
table is the reference program's, byte for byte; (c) LD decay's bins and (d) LD pruning's sets equal what the scripts' rules
make of the REFERENCE program's table (not the engine's own, which a wrong device value would bend the same way); so do (e) the
per-site LD summaries and (f) the LD clusters, whose sums, maxima and counts are integers of printed micro-units: with
linked_min / min_weight on a value a tie prints (and on the value the other rounding would print), the maf filter at equality,
on both accumulation paths, in small chunks, (g) on the generic pair kernels too, and (h) as the binary's files.  Every case
first asserts that it holds the ties it is about, and every threshold that the reference table has rows exactly on it."""
import ctypes as C
import gzip
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cluster_ref
import decay_ref
import prune_ref
import site_ref
from ngsld_amd import capi, shard, synth
from oracle import orc
from printed_values import is_tie, micro
from test_gpu_clusters import _same as same_clusters
from test_gpu_decay import _same as same_bins
from test_gpu_site_ld import _same as same_sites
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
        self.name = name
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


# ---- (e) - (h): per-site LD and LD clusters.  A threshold is held as q, the micro-units "%f" prints of it; the double handed to
# the engine, the restatements and the binary is q / 10^6, what a reader makes of that text (site_ref.printed).
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
KBS = (math.inf, 3.0, 1.0, 0.5)
SITE_KNOBS = ("NGSLD_TEST_SITE_LDS_BYTES", "NGSLD_TEST_SITE_CHUNK_PAIRS")
CLUSTER_KNOB = "NGSLD_TEST_CLUSTER_CHUNK_PAIRS"


def _small(case):
    if case.kind == "call_geno" or case.n_ind > 16:
        pytest.skip("site LD and clusters run on the called cohorts of 8 and 16 and the text file")


def _ties(case):
    """The distinct tie |D| of the oracle's records, commonest first, as [(q, up)]: q the micro-units "%f" prints of it (half to
    even), up whether that rounds the tie up -- then the raw double lies BELOW q / 10^6."""
    vals, counts = np.unique(np.abs(case.rec["D"][case.d_ties]), return_counts=True)
    vals = [float(vals[k]) for k in np.argsort(-counts, kind="stable")]
    return [(micro(v), micro(v) > Fraction(v) * 10 ** 6) for v in vals]


def _other(q, up):
    """The tie's other neighbour: what a rounder that takes it the other way prints, on the far side of the raw double."""
    return q - 1 if up else q + 1


def _floors(case):
    """The commonest tie |D|, the commonest that rounds up and the commonest that rounds down (two or three of them)."""
    ties = _ties(case)
    ups, downs = [t for t in ties if t[1]], [t for t in ties if not t[1]]
    assert ups and downs, ties
    return list(dict.fromkeys([ties[0], ups[0], downs[0]]))


def _ref_rows(case, text):
    """The rows of the reference program's table with a finite dist and D, as arrays (site1, site2, |D| in micro-units, dist):
    what the thresholds are counted on, and what the search of _structured runs over."""
    if not hasattr(case, "rows"):
        index = {lab: k for k, lab in enumerate(case.labels)}
        out = []
        for ln in text.splitlines():
            f = ln.split("\t")
            if not ln or f[0] == "site1" or f[2].strip().lstrip("+-").lower() in ("inf", "nan"):
                continue
            q = site_ref.micro(f[4])
            if q is not None:
                out.append((index[f[0]], index[f[1]], abs(q), int(f[2])))
        case.rows = tuple(np.array(out, dtype=np.int64).T)
    return case.rows


def _on(rows, q, kb=math.inf):
    """Rows within kb whose |D| prints exactly q: the boundary rows of a floor q / 10^6."""
    return int(np.count_nonzero((rows[2] == q) & (rows[3] <= kb * 1000)))


def _from(rows, q, kb=math.inf):
    return int(np.count_nonzero((rows[2] >= q) & (rows[3] <= kb * 1000)))


def _components(n, a, b):
    """Every site's smallest connected site over the edges (a[k], b[k]) (numpy: only the search below uses it)."""
    lab = np.arange(n)
    while True:
        new = lab.copy()
        low = np.minimum(lab[a], lab[b])
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def _structured(case, text):
    """(q, up, kb): a tie floor x max_kb_dist of KBS, ties commonest first, with an edge exactly on the floor that leaves at least
    three clusters of three sites and a singleton -- the first at which the components change when the floor moves one
    micro-unit up if there is one, else the first of all.  Where no setting has that shape (text_n8_missing: near pairs are in
    strong LD there, and within 3 kb only the two highest tie floors, with one and five edges on them, leave more than one
    cluster of three sites) the one with an edge on the floor and the most clusters of three sites, then the most edges on it.
    None without any.  A search: the test then asserts what it found with the restatement."""
    if not hasattr(case, "structured"):
        s1, s2, qd, dist = _ref_rows(case, text)
        first, best = None, None
        for q, up in _ties(case):
            for kb in KBS:
                near = dist <= kb * 1000
                on = int(np.count_nonzero(near & (qd == q)))
                if not on:
                    continue
                lab = _components(N_SITES, s1[near & (qd >= q)], s2[near & (qd >= q)])
                size = np.bincount(lab, minlength=N_SITES)
                big, single = int(np.count_nonzero(size >= 3)), int(np.count_nonzero(size == 1))
                if single >= 1 and (best is None or (big, on) > best[0]):
                    best = ((big, on), (q, up, kb))
                if big < 3 or single < 1:
                    continue
                first = first or (q, up, kb)
                if not np.array_equal(lab, _components(N_SITES, s1[near & (qd > q)], s2[near & (qd > q)])):
                    case.structured = (q, up, kb)
                    return case.structured
        case.structured = first or (best and best[1])
    return case.structured


def _cached(fn, text, labels, **fixed):
    """fn(text, labels, **fixed, **kw), computed once per kw: the restatements take a moment over 44,850 rows."""
    seen = {}

    def want(**kw):
        key = tuple(sorted(kw.items()))
        if key not in seen:
            seen[key] = fn(text, labels, **fixed, **kw)
        return seen[key]
    return want


@needs_ref
def test_site_ld_of_the_reference_table(case, monkeypatch):
    """(e) per-site LD on the device against the rule of SITES.md on the reference program's table, integers equal and means
    bit for bit: all four statistics signed and absolute, with the LDS and the global accumulators and in chunks of 3,000
    pairs; linked_min on the value a tie prints and on the one the other rounding would print; min_maf a printed frequency;
    a distance limit inside the data.  (g) called_n8 once more on the generic pair kernels."""
    _small(case)
    text = _ref_table(case, True, os.path.dirname(case.ppath))
    rows = _ref_rows(case, text)
    floors = _floors(case)
    top = floors[0][0] / 10 ** 6
    min_maf = 1.0 / case.n_ind
    assert f"\t{min_maf:f}\t" in text
    want = _cached(site_ref.site_ld, text, case.labels)
    for k in SITE_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("NGSLD_TEST_HARD_KERNEL", raising=False)

    def check(eng, **kw):
        sites, stats = eng.site_ld(**kw)
        w = want(**kw)
        same_sites(sites, w, kw["ld"])
        assert stats["pairs"] == len(case.rec) and stats["pairs_counted"] * 2 == sum(w["n"]) > 0
        return stats, w

    all4 = dict(ld=ALL4, linked_min=top, abs_value=False)
    eng = case.engine()
    try:
        eng.plan(extend_out=True)
        st, signed = check(eng, **all4)
        assert st["lds"] == 1
        monkeypatch.setenv(SITE_KNOBS[0], "0")
        assert check(eng, **all4)[0]["lds"] == 0
        monkeypatch.delenv(SITE_KNOBS[0])
        monkeypatch.setenv(SITE_KNOBS[1], "3000")
        st, _ = check(eng, **all4)
        assert st["lds"] == 1 and st["chunks"] > 5
        monkeypatch.delenv(SITE_KNOBS[1])
        _, absolute = check(eng, ld=ALL4, linked_min=top, abs_value=True)
        assert signed["sum_D"] != absolute["sum_D"] and signed["linked_D"] != absolute["linked_D"]  # (negative D, some beyond -top)
        notes = []
        for q, up in floors:
            _, w = check(eng, ld=("D",), linked_min=q / 10 ** 6)
            _, o = check(eng, ld=("D",), linked_min=_other(q, up) / 10 ** 6)
            on, linked, other = _on(rows, q), sum(w["linked_D"]), sum(o["linked_D"])
            assert on > 0 and linked == 2 * _from(rows, q)
            # rounded down: the other neighbour lies above, the boundary rows are linked at q and not at q + 1; rounded up: it
            # lies below, and they are linked at both
            assert (other - linked == 2 * _on(rows, q - 1)) if up else (linked - other == 2 * on)
            notes.append(f"{q / 10 ** 6:f} ({'up' if up else 'down'}, {on} rows on it, linked ends {linked} / {other} at its other neighbour)")
        check(eng, ld=("D",), linked_min=top, min_maf=min_maf)
        _, w = check(eng, ld=("D", "r2"), linked_min=top, max_kb_dist=1.0)
        assert 0 < sum(w["n"]) < sum(absolute["n"])
    finally:
        eng.close()
    print(f"site LD: linked_min on the printed ties {'; '.join(notes)}; min_maf {min_maf:f}; equal to the rule on the reference table")
    if case.name == "called_n8":
        monkeypatch.setenv("NGSLD_TEST_HARD_KERNEL", "0")
        eng = case.engine()
        try:
            assert eng.pair_kernel() != "hard"
            eng.plan(extend_out=True)
            check(eng, **all4)
        finally:
            eng.close()
        print("site LD: the same on the generic pair kernels")


def _edges(table):
    return sum(r["edges"] for r in table)


def _shape(table):
    return sum(1 for r in table if r["size"] >= 3), sum(1 for r in table if r["size"] == 1)


@needs_ref
def test_clusters_of_the_reference_table(case, monkeypatch):
    """(f) LD clusters on D (field 5) on the device against the rule of CLUSTERS.md on the reference program's table, ids and
    integers equal, means and densities bit for bit: the floor on the commonest printed tie |D|; a structured setting (a tie floor
    and a distance limit that leave three clusters of three sites, a singleton and edges exactly on the floor -- for called_n8 one
    whose ids change without those edges); the floors the other rounding would print; signed D; min_maf a printed frequency;
    chunks of 3,000 pairs; LD pruning's graph of the same setting.  (g) called_n8 once more on the generic pair kernels."""
    _small(case)
    text = _ref_table(case, True, os.path.dirname(case.ppath))
    rows = _ref_rows(case, text)
    min_maf = 1.0 / case.n_ind
    assert f"\t{min_maf:f}\t" in text
    want = _cached(cluster_ref.clusters, text, case.labels, min_size=1, field=5)
    monkeypatch.delenv(CLUSTER_KNOB, raising=False)
    monkeypatch.delenv("NGSLD_TEST_HARD_KERNEL", raising=False)

    def check(eng, **kw):
        ids, table, stats = eng.clusters(field=5, min_size=1, **kw)
        w_ids, w_table = want(**kw)
        same_clusters(ids, table, w_ids, w_table)
        assert stats["pairs"] == len(case.rec) and stats["edges"] == _edges(w_table) > 0
        assert stats["nodes"] == sum(1 for k in w_ids if k) and stats["clusters"] == len(w_table)
        return ids, stats

    # the settings and what the reference table holds at them, before the device is asked
    top = _floors(case)[0][0]
    assert _on(rows, top) > 0 and _edges(want(min_weight=top / 10 ** 6)[1]) == _from(rows, top)
    found = _structured(case, text)
    assert found is not None, "no tie floor leaves a singleton and has an edge on it"
    q, up, kb = found
    floor = q / 10 ** 6
    here = dict(min_weight=floor, max_kb_dist=kb)
    w_ids, w_table = want(**here)
    above_ids, above_table = want(min_weight=(q + 1) / 10 ** 6, max_kb_dist=kb)
    on, (big, single) = _on(rows, q, kb), _shape(w_table)
    assert on > 0 and _edges(w_table) == _from(rows, q, kb) == _edges(above_table) + on
    # (the text file has no tie floor of that shape -- _structured -- and is held to more than one cluster of three sites)
    assert big >= (3 if case.kind == "bin" else 2) and single >= 1, (big, single)
    ids_change = w_ids != above_ids
    assert ids_change or case.name != "called_n8"
    q2, up2 = next(t for t in _ties(case) if t[1] != up and _on(rows, t[0], kb) > 0)   # (a tie that rounds the other way)
    print(f"clusters: floor {top / 10 ** 6:f} with {_on(rows, top)} of {_from(rows, top)} edges on it; structured setting "
          f"{floor:f} ({'up' if up else 'down'}) at {kb} kb: {len(w_table)} clusters ({big} of three sites, {single} singletons), "
          f"{on} of {_edges(w_table)} edges on the floor, ids {'change' if ids_change else 'stay'} without them; other neighbours "
          f"{_other(q, up) / 10 ** 6:f} and {_other(q2, up2) / 10 ** 6:f} ({_on(rows, q2, kb)} edges on {q2 / 10 ** 6:f})")

    eng = case.engine()
    try:
        eng.plan(extend_out=True)
        check(eng, min_weight=top / 10 ** 6)
        ids, st = check(eng, **here)
        check(eng, min_weight=_other(q, up) / 10 ** 6, max_kb_dist=kb)
        check(eng, min_weight=_other(q2, up2) / 10 ** 6, max_kb_dist=kb)
        check(eng, abs_value=False, **here)
        assert 0 < _edges(want(abs_value=False, **here)[1]) < _edges(w_table)   # (negative D beyond -floor)
        check(eng, min_maf=min_maf, **here)
        monkeypatch.setenv(CLUSTER_KNOB, "3000")
        assert check(eng, **here)[1]["chunks"] > 5
        monkeypatch.delenv(CLUSTER_KNOB)
        state, pst = eng.prune(case.labels, field=5, weight_type="a", min_weight=floor, max_kb_dist=kb)
        assert pst["edges"] == st["edges"] == _edges(w_table) and np.array_equal(state != 0, ids != 0)
        assert pst["nodes"] == st["nodes"] == sum(1 for k in w_ids if k)
    finally:
        eng.close()
    if case.name == "called_n8":
        monkeypatch.setenv("NGSLD_TEST_HARD_KERNEL", "0")
        eng = case.engine()
        try:
            assert eng.pair_kernel() != "hard"
            eng.plan(extend_out=True)
            check(eng, **here)
        finally:
            eng.close()
        print("clusters: the same on the generic pair kernels")


@needs_ref
def test_site_and_cluster_files_of_the_reference_table(case, tmp_path):
    """(h) one run of the binary: --site_out, --cluster_out and --cluster_table, linked_min and the floor on printed ties, are
    the files the restatements write from the reference program's table, byte for byte."""
    if case.name not in ("called_n8", "text_n8_missing"):
        pytest.skip("the binary's files are checked on the called cohort of 8 and the text file")
    text = _ref_table(case, True, os.path.dirname(case.ppath))
    rows = _ref_rows(case, text)
    top = _floors(case)[0][0]
    q, _, kb = _structured(case, text)
    assert _on(rows, top) > 0 and _on(rows, q, kb) > 0
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_")}
    s, c, k = (str(tmp_path / f) for f in ("s.tsv", "c.tsv", "k.tsv"))
    h = subprocess.run([capi.CLI_PATH, *case.flags, "--extend_out", "--n_threads", "2",
                        "--site_out", s, "--site_ld", "D,r2", "--site_linked_min", repr(top / 10 ** 6),
                        "--cluster_out", c, "--cluster_table", k, "--cluster_field", "5", "--cluster_min_weight", repr(q / 10 ** 6),
                        "--cluster_max_kb_dist", repr(kb), "--cluster_min_size", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert h.returncode == 0, h.stderr[-2000:]
    assert open(s).read() == site_ref.site_file(text, case.labels, ld=("D", "r2"), linked_min=top / 10 ** 6)
    ids, table = cluster_ref.clusters(text, case.labels, min_size=1, field=5, min_weight=q / 10 ** 6, max_kb_dist=kb)
    assert open(c).read() == cluster_ref.cluster_file(ids, case.labels)
    assert open(k).read() == cluster_ref.table_file(table, case.labels)
    print(f"files: linked_min {top / 10 ** 6:f} ({_on(rows, top)} rows on it), floor {q / 10 ** 6:f} at {kb} kb ({_on(rows, q, kb)} edges "
          f"on it): {N_SITES} sites and {len(table)} clusters identical")
