"""LD partners on the device (ngsld_partners, Engine.partners, the binary's --partners_* flags) against tests/partners_ref.py --
the rule of PARTNERS.md in plain Python, integers only -- applied to the same engine's own full table (Engine.run + run_text, as
tests/test_gpu_linked.py's Table builds it).  Every array and file must be equal as bytes: nothing sampled, no tolerance.

The shapes are the smallest at which the kernel can still go wrong: rows longer than 64 candidates (a row spans items), row tails
shorter than 64, masks with holes (rnd_sample), more than one chromosome, sites with more and with fewer partner rows than k,
every site's slots hit from many wavefronts at once (all pairs, no floor), ties at the k-th place, chunks and slices that cut
between the items of one row -- 300 to 500 sites, 8 / 64 / 500 individuals, a 20 kb window over gaps of up to 300 bp.

GPU time of this file on one MI355X: see PARTNERS.md ("What the tests cost")."""
import math
import os
import subprocess

import numpy as np
import pytest

import partners_ref
from ngsld_amd import capi, shard, synth
from test_gpu_linked import CASES as LINKED_CASES, Table, _chunks, _engine, _labels
from util import have_ref_program

pytestmark = pytest.mark.gpu

KNOBS = ("NGSLD_TEST_PARTNERS_CHUNK_PAIRS", "NGSLD_TEST_PARTNERS_PLANT_DP", "NGSLD_TEST_RECORD_SLICE_ITEMS")
INF = math.inf
WIN = dict(max_kb_dist=20, extend_out=True)
KS = (1, 5, 64)


def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _want(tab, n_sites, query=None, **kw):
    """The rule at k = 64 on the table, once per setting; a smaller k is its first columns (the first k of a ranked list)."""
    key = (None if query is None else bytes(np.asarray(query, dtype=np.uint8)), tuple(sorted(kw.items())))
    cache = tab.__dict__.setdefault("_partners", {})
    if key not in cache:
        cache[key] = partners_ref.partners(tab.text, tab.s1, tab.s2, n_sites, 64, query=query, label_cols=tab.label_cols,
                                           maf=tab.maf, **kw)
    return cache[key]


def _check(eng, tab, k, query=None, **kw):
    """Engine.partners at k against the rule, as bytes; returns (result, stats)."""
    n = eng.n_sites
    rows, partner, value = _want(tab, n, query, **kw)
    res, st = eng.partners(k, query=query, **kw)
    assert res["rows"].dtype == np.uint64 and res["rows"].tobytes() == rows.tobytes()
    assert res["partner"].dtype == np.int64 and res["partner"].shape == (n, k)
    assert res["partner"].tobytes() == np.ascontiguousarray(partner[:, :k]).tobytes()
    assert res["value_micro"].dtype == np.int64 and res["value_micro"].tobytes() == np.ascontiguousarray(value[:, :k]).tobytes()
    none = partner[:, :k] < 0
    assert res["value"].dtype == np.float64 and np.array_equal(np.isnan(res["value"]), none)
    assert np.array_equal(res["value"][~none], (value[:, :k] / 1e6)[~none])
    all_rows = _want(tab, n, None, **kw)[0]
    assert st["pairs"] == len(tab.rows) and st["rows_counted"] * 2 == int(all_rows.sum())
    assert st["sites_with_partners"] == int((rows > 0).sum()) and st["entries"] == int((~none).sum())
    print(f"k {k} pairs {st['pairs']} partner rows {st['rows_counted']} sites {st['sites_with_partners']} entries {st['entries']} "
          f"rows/site max {int(rows.max())} min {int(rows.min())} chunks {st['chunks']} pairs_ms {st['pairs_ms']:.2f} "
          f"kernel_ms {st['kernel_ms']:.3f} total_ms {st['total_ms']:.2f}")
    return res, st


# ---- 1: the cases of the linked pairs, each at k = 1, 5 and 64 ----
@pytest.mark.parametrize("name", list(LINKED_CASES))
def test_partners_equal_the_rule_on_own_table(name, monkeypatch):
    _no_knobs(monkeypatch)
    n_sites, n_ind, skw, n_chr, plan_kw, kw, geno_kw = LINKED_CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 500 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 37, max_gap=300, n_chr=n_chr)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        row_off, _ = eng.plan_rows()
        assert int(np.diff(row_off).max()) > 64 or name == "max_snp_dist"  # (a row spans items; 40 candidates a row there)
        tab = Table(eng, _labels(chrs, pos))
        more, fewer = {}, {}
        for k in KS:
            res, st = _check(eng, tab, k, **kw)
            assert st["chunks"] == 1 and 0 < st["rows_counted"] < st["pairs"]
            more[k], fewer[k] = int((res["rows"] > k).sum()), int((res["rows"] < k).sum())
        print(f"{name}: sites with more than k partner rows {more}, with fewer {fewer}")
        # a list that is cut (at the smallest k) and a list that stays short (at the largest, if not before).  The negative
        # floor on the signed D passes nearly every row of the window: there every list is cut, at k = 64 too
        assert more[1] > 0 and (max(fewer.values()) > 0 or name == "signed_D_negative_floor")
        if name == "signed_D_negative_floor":
            assert more[64] == n_sites
    finally:
        eng.close()


# ---- 2: contention and ties ----
@pytest.mark.parametrize("how", ["n64", "n8_call_geno"])
def test_every_site_fed_by_many_wavefronts(how, monkeypatch):
    """All pairs of 300 sites, no floor, signed: every site has 299 candidates, which arrive from its own row's items and from
    the rows of every site before it.  With called genotypes of 8 individuals many printed values tie, at the k-th place too."""
    _no_knobs(monkeypatch)
    n_ind, geno_kw = (64, None) if how == "n64" else (8, dict(call_geno=(0.1, 0.9)))
    raw = synth.make_gl_numpy(300, n_ind, 864 + n_ind, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300)
    eng = _engine(raw, chrs, pos, dict(extend_out=True), geno_kw)
    try:
        tab = Table(eng, _labels(chrs, pos))
        assert len(tab.rows) == 300 * 299 // 2
        kw = dict(field=5, min_weight=-INF, abs_value=False)
        res, st = _check(eng, tab, 5, **kw)
        assert (res["rows"] == 299).all() and st["entries"] == 300 * 5
        if how == "n8_call_geno":
            value = _want(tab, 300, None, **kw)[2]
            tied = int((value[:, 4] == value[:, 5]).sum())
            print(f"sites whose 5th and 6th values are equal: {tied}")
            assert tied > 0
    finally:
        eng.close()


# ---- 3: chunks and slices ----
def test_chunks_and_slices_give_the_same_bytes(monkeypatch):
    _no_knobs(monkeypatch)
    raw = synth.make_gl_numpy(500, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 71, max_gap=300, n_chr=2)
    eng = _engine(raw, chrs, pos, dict(max_kb_dist=20, extend_out=True, rnd_sample=0.8, seed=3))
    kw = dict(min_weight=0.1)
    try:
        tab = Table(eng, _labels(chrs, pos))
        row_off = [int(x) for x in eng.plan_rows()[0]]
        n_pairs = row_off[-1]
        base, st0 = _check(eng, tab, 5, **kw)
        assert st0["chunks"] == 1 and len(eng.items()) > 3 * 64
        tenth = n_pairs // 10
        runs = {
            "tenth": {"NGSLD_TEST_PARTNERS_CHUNK_PAIRS": str(tenth)},
            "row": {"NGSLD_TEST_PARTNERS_CHUNK_PAIRS": "1"},
            "slice64": {"NGSLD_TEST_RECORD_SLICE_ITEMS": "64"},
            "slice7": {"NGSLD_TEST_RECORD_SLICE_ITEMS": "7"},
            "tenth_slice7": {"NGSLD_TEST_PARTNERS_CHUNK_PAIRS": str(tenth), "NGSLD_TEST_RECORD_SLICE_ITEMS": "7"},
        }
        for name, env in runs.items():
            _no_knobs(monkeypatch)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            res, st = _check(eng, tab, 5, **kw)
            assert all(res[k].tobytes() == base[k].tobytes() for k in ("rows", "partner", "value_micro")), name
            want = _chunks(row_off, int(env.get("NGSLD_TEST_PARTNERS_CHUNK_PAIRS", n_pairs)))
            assert st["chunks"] == len(want), (name, st["chunks"], len(want))
            if name == "tenth":
                assert len(want) > 10
            if name == "row":
                assert len(want) == sum(1 for a, b in zip(row_off, row_off[1:]) if b > a) > 400
    finally:
        _no_knobs(monkeypatch)
        eng.close()


# ---- 4: agreement with the linked pairs ----
def test_lists_are_the_linked_pairs_in_both_directions(monkeypatch):
    """max_snp_dist=30: a site has at most 30 partners to each side, so k = 64 cuts no list and the lists hold every linked row
    once from each end."""
    _no_knobs(monkeypatch)
    raw = synth.make_gl_numpy(500, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 71, max_gap=300, n_chr=2)
    eng = _engine(raw, chrs, pos, dict(max_snp_dist=30, extend_out=True))
    try:
        for kw in (dict(field=7, min_weight=0.05), dict(field=5, min_weight=-0.01, abs_value=False, min_maf=0.05)):
            res, st = eng.partners(64, **kw)
            link, lst = eng.linked_pairs(None, records=True, **kw)
            assert lst["rows"] == st["rows_counted"] > 500 and int(res["rows"].max()) <= 60
            name = {5: "D", 7: "r2"}[kw["field"]]
            q = np.array([partners_ref.micro(f"{x:f}") for x in link["std"][name]], dtype=np.int64)
            if kw.get("abs_value", True):
                q = np.abs(q)
            a, b = link["s1"].astype(np.int64), link["s2"].astype(np.int64)
            want = set(zip(a.tolist(), b.tolist(), q.tolist())) | set(zip(b.tolist(), a.tolist(), q.tolist()))
            s, j = np.nonzero(res["partner"] >= 0)
            got = set(zip(s.tolist(), res["partner"][s, j].tolist(), res["value_micro"][s, j].tolist()))
            assert got == want and len(got) == 2 * lst["rows"]
            assert np.array_equal(res["rows"], np.bincount(np.concatenate([a, b]), minlength=500).astype(np.uint64))
    finally:
        eng.close()


# ---- 5: a query ----
def test_a_query_collects_for_its_sites_only(monkeypatch):
    _no_knobs(monkeypatch)
    raw = synth.make_gl_numpy(400, 64, 964, depth=4.0)
    chrs, pos = synth.make_positions(400, 37, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, _labels(chrs, pos))
        kw = dict(min_weight=0.2)
        full, _ = _check(eng, tab, 5, **kw)
        mask = np.random.default_rng(5).random(400) < 0.1
        assert 20 < mask.sum() < 80
        res, st = _check(eng, tab, 5, query=mask, **kw)
        for k in ("rows", "partner", "value_micro"):
            assert np.array_equal(res[k][mask], full[k][mask]), k
        assert (res["rows"][~mask] == 0).all() and (res["partner"][~mask] == -1).all() and (res["value_micro"][~mask] == 0).all()
        assert (~mask[res["partner"][res["partner"] >= 0]]).any()  # (a partner outside the query)
        res, st = _check(eng, tab, 5, query=np.zeros(400, dtype=np.uint8), **kw)
        assert st["entries"] == 0 and st["sites_with_partners"] == 0 and st["rows_counted"] > 0
        assert (res["partner"] == -1).all() and not res["rows"].any()
    finally:
        eng.close()


# ---- 6: the range ----
def test_a_planted_dp_of_2_31_micro_units_is_refused_naming_the_pair(monkeypatch):
    """Valid haplotype frequencies give no finite D' near 2147.483648, so NGSLD_TEST_PARTNERS_PLANT_DP writes one into the record
    buffer: the largest value allowed is kept and ranked first, the first one beyond is refused with the pair's name and leaves
    no result; in a row the maf filter drops it is not read."""
    _no_knobs(monkeypatch)
    raw = synth.make_gl_numpy(300, 64, 3, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, _labels(chrs, pos))
        at = len(tab.rows) // 2
        a, b = int(tab.s1[at]), int(tab.s2[at])
        lines = tab.text.splitlines(keepends=True)

        def planted(value):
            f = lines[at].split("\t")
            f[5] = value
            t = Table.__new__(Table)
            t.__dict__.update({k: v for k, v in tab.__dict__.items() if k != "_partners"})
            t.text = "".join(lines[:at] + ["\t".join(f)] + lines[at + 1:])
            t.rows = t.text.splitlines()
            return t

        kw = dict(field=6, min_weight=0.9)
        for value in ("2147.483647", "-2147.483647"):
            monkeypatch.setenv("NGSLD_TEST_PARTNERS_PLANT_DP", f"{at}:{value}")
            res, _ = _check(eng, planted(value), 5, **kw)
            assert res["partner"][a, 0] == b and res["partner"][b, 0] == a and res["value_micro"][a, 0] == 2147483647
        monkeypatch.setenv("NGSLD_TEST_PARTNERS_PLANT_DP", f"{at}:-2147.483647")
        res, _ = _check(eng, planted("-2147.483647"), 5, field=6, min_weight=-INF, abs_value=False)
        assert res["value_micro"][a, -1] != -2147483647 and res["rows"][a] > 5  # (signed: the smallest value, cut away)
        for value in ("2147.483648", "-2147.483648", "1e300"):
            monkeypatch.setenv("NGSLD_TEST_PARTNERS_PLANT_DP", f"{at}:{value}")
            with pytest.raises(partners_ref.RangeError) as r:
                partners_ref.partners(planted(f"{float(value):f}").text, tab.s1, tab.s2, 300, 5, **kw)
            assert r.value.pair == (a, b)
            with pytest.raises(capi.NgsldError) as e:
                eng.partners(5, **kw)
            assert e.value.code == capi.ERR_UNSUPPORTED and f"the pair of sites {a} - {b} reaches 2^31 micro-units" in e.value.msg
            info = eng._L.ngsld_partners_info(eng._h, None, None, None)
            assert info == capi.ERR_INVALID and b"no ngsld_partners result" in eng._L.ngsld_last_error(eng._h)
            eng.partners(5, field=7)  # (D' is not chosen: the planted value is not read)
            # a row the maf filter drops: above the larger of the pair's printed maf
            floor = max(tab.maf[tab.labels[a]], tab.maf[tab.labels[b]]) + 1e-6
            _check(eng, planted(f"{float(value):f}"), 5, min_maf=floor, **kw)
        monkeypatch.delenv("NGSLD_TEST_PARTNERS_PLANT_DP")
        _check(eng, tab, 5, **kw)  # (the context stays usable)
    finally:
        _no_knobs(monkeypatch)
        eng.close()


# ---- 7: refusals ----
def test_refusals(monkeypatch):
    import ctypes as C
    _no_knobs(monkeypatch)
    raw = synth.make_gl_numpy(300, 16, 3, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300)
    U, I = capi.ERR_UNSUPPORTED, capi.ERR_INVALID

    def refused(eng, code, *words, k=5, **kw):
        with pytest.raises(capi.NgsldError) as e:
            eng.partners(k, **kw)
        assert e.value.code == code and all(w in e.value.msg for w in words), (e.value.code, e.value.msg)
        assert eng._L.ngsld_partners_info(eng._h, None, None, None) == I  # (a failure leaves no result)

    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        refused(eng, I, "ngsld_plan has not been called")
        eng.plan(**WIN)
        assert eng.partners(5, min_weight=0.2)[1]["entries"] > 0
        for k in (0, 65):
            refused(eng, I, "partners k must be in 1..64", k=k)
        for f in (3, 8):
            refused(eng, I, "partners field must be a TSV column 4..7", field=f)
        refused(eng, I, "min_weight is NaN", min_weight=math.nan)
        refused(eng, I, "max_kb_dist", max_kb_dist=math.nan)
        refused(eng, I, "max_kb_dist", max_kb_dist=-1.0)
        refused(eng, I, "min_maf is NaN", min_maf=math.nan)
        p = capi.PartnersParams(C.sizeof(capi.PartnersParams) - 8, 5, 7, 1, 0.5, INF, 0.0)
        assert eng._L.ngsld_partners(eng._h, C.byref(p), None, None) == I and b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = capi.PartnersParams(C.sizeof(capi.PartnersParams), 5, 7, 1, 0.5, INF, 0.0)
        st = capi.PartnersStats()  # (struct_size not set)
        assert eng._L.ngsld_partners(eng._h, C.byref(p), None, C.byref(st)) == I
        assert eng._L.ngsld_partners(eng._h, C.byref(p), None, None) == capi.OK  # (stats may be NULL)
        k, n, f = C.c_uint32(), C.c_uint64(), C.c_uint32()
        assert eng._L.ngsld_partners_info(eng._h, C.byref(k), C.byref(n), C.byref(f)) == capi.OK
        assert (k.value, n.value, f.value) == (5, 300, 7)
        eng.plan(**WIN)  # the store goes with the next plan
        assert eng._L.ngsld_partners_info(eng._h, None, None, None) == I
        assert eng._L.ngsld_partners_get(eng._h, None, None, None) == I
        # positions no file holds: half a base between sites.  A finite limit is refused; without one the call goes through
        eng.set_pos_dist(np.full(300, 10.5))
        eng.plan(max_kb_dist=1, extend_out=True)
        refused(eng, U, "partners max_kb_dist needs integer position gaps", max_kb_dist=0.5)
        assert eng.partners(5, min_weight=0.1)[1]["entries"] > 0
        # no planned pair: empty lists, no error
        eng.set_pos_dist(np.full(300, 5000.0))
        assert eng.plan(max_kb_dist=1, extend_out=True) == 0
        res, st = eng.partners(3)
        assert st["pairs"] == 0 and st["chunks"] == 0 and not res["rows"].any() and (res["partner"] == -1).all()
        assert res["partner"].shape == (300, 3)
    finally:
        eng.close()


# ---- 8: the binary ----
def test_cli_partners_out(tmp_path):
    n_sites, n_ind = 400, 64
    raw = synth.make_gl_numpy(n_sites, n_ind, 97, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 97, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    geno = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "20", "--extend_out"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, base=geno + ["--pos", p], env=env: subprocess.run([*base, *a], capture_output=True, text=True,  # noqa: E731
                                                                       cwd=str(tmp_path), timeout=300, env=env)
    # next to --out in one run: the file is the rule over that run's table
    r = run("--out", "t.tsv", "--partners_out", "a.tsv", "--partners_k", "5", "--partners_min_weight", "0.2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "==> LD partners:" in r.stderr
    table = open(tmp_path / "t.tsv").read()
    index = {lab: k for k, lab in enumerate(labels)}
    rows = partners_ref.rows_of(table)
    s1 = [index[ln.split("\t")[0]] for ln in rows]
    s2 = [index[ln.split("\t")[1]] for ln in rows]

    def want(k, names=labels, **kw):
        _, partner, value = partners_ref.partners(table, s1, s2, n_sites, k, **kw)
        return partners_ref.partners_file(partner, value, names, kw.get("field", 7))

    text = open(tmp_path / "a.tsv").read()
    assert text == want(5, min_weight=0.2) and text.startswith("site\trank\tpartner\tr2\n") and len(text.splitlines()) > 500
    # alone: no TSV (not even on standard output); the other flags
    r = run("--partners_out", "b.tsv", "--partners_k=3", "--partners_field", "5", "--partners_signed", "--partners_min_weight=-0.01",
            "--partners_max_kb_dist", "7.5", "--partners_min_maf", "0.05")
    assert r.returncode == 0 and r.stdout == "", r.stderr[-2000:]
    text = open(tmp_path / "b.tsv").read()
    assert text == want(3, field=5, abs_value=False, min_weight=-0.01, max_kb_dist=7.5, min_maf=0.05)
    assert text.startswith("site\trank\tpartner\tD\n") and text != want(3, field=5, min_weight=0.01, max_kb_dist=7.5, min_maf=0.05)
    # a query by label; an unknown label
    some = [labels[k] for k in (3, 77, 250, 399)]
    (tmp_path / "q.txt").write_text("".join(s + "\n" for s in some))
    r = run("--partners_out", "c.tsv", "--partners_k", "64", "--partners_min_weight", "0.2", "--partners_sites", "q.txt")
    assert r.returncode == 0, r.stderr[-2000:]
    query = np.zeros(n_sites, dtype=np.uint8)
    query[[3, 77, 250, 399]] = 1
    text = open(tmp_path / "c.tsv").read()
    assert text == want(64, min_weight=0.2, query=query) and {ln.split("\t")[0] for ln in text.splitlines()[1:]} <= set(some)
    assert len(text.splitlines()) > 4
    (tmp_path / "q2.txt").write_text(some[0] + "\nchr9:1\n")
    r = run("--partners_out", "d.tsv", "--partners_k", "5", "--partners_sites", "q2.txt")
    assert r.returncode == 255 and "ERROR" in r.stderr and "chr9:1" in r.stderr, r.stderr[-1000:]
    # without --pos (and so without a window: all pairs, every dist inf): sites by their 1-based index
    r = run("--partners_out", "e.tsv", "--partners_k", "5", "--partners_min_weight", "0.2", "--out", "t2.tsv",
            base=geno[:-3] + ["--max_kb_dist", "0", "--extend_out"])
    assert r.returncode == 0, r.stderr[-2000:]
    table2 = open(tmp_path / "t2.tsv").read()
    rows2 = partners_ref.rows_of(table2)
    a = [int(ln.split("\t")[0]) - 1 for ln in rows2] if rows2[0].split("\t")[0].isdigit() else None
    if a is None:  # (the table names a site without a label "(null)": the pairs in plan order)
        a, b = zip(*[(i, j) for i in range(n_sites) for j in range(i + 1, n_sites)])
    else:
        b = [int(ln.split("\t")[1]) - 1 for ln in rows2]
    assert len(a) == len(rows2)
    _, partner, value = partners_ref.partners(table2, a, b, n_sites, 5, min_weight=0.2)
    assert open(tmp_path / "e.tsv").read() == partners_ref.partners_file(partner, value, [str(k + 1) for k in range(n_sites)])
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--partners_out", "f.tsv", "--partners_k", "5", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--partners_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "f.tsv")


# ---- 9: ties of the reference program's table ----
def test_lists_on_printed_ties_of_the_reference_table(tmp_path, monkeypatch):
    """The tie-heavy input of tests/test_gpu_ties.py: 300 sites, called genotypes of 8 and 16 individuals, all pairs, D.  Expected =
    the rule over the REFERENCE program's table (which a wrong device value could not bend): a value one micro-unit off at a
    "%f" tie would change a rank, a floor on the tie's value a list."""
    import test_gpu_ties as ties
    if not have_ref_program():
        pytest.skip("oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")
    _no_knobs(monkeypatch)
    for name in ("called_n8", "called_n16"):
        d = str(tmp_path / name)
        os.makedirs(d)
        case = ties.Case(name, d)
        text = ties._ref_table(case, True, d)
        index = {lab: k for k, lab in enumerate(case.labels)}
        rows = partners_ref.rows_of(text)
        s1 = [index[ln.split("\t")[0]] for ln in rows]
        s2 = [index[ln.split("\t")[1]] for ln in rows]
        ref_rows = ties._ref_rows(case, text)
        eng = case.engine()
        try:
            eng.plan(extend_out=True)
            for q, up in ties._floors(case):
                assert ties._on(ref_rows, q) > 0  # rows exactly on the floor
                for floor in (q, ties._other(q, up)):
                    kw = dict(field=5, min_weight=floor / 10 ** 6)
                    want = partners_ref.partners(text, s1, s2, ties.N_SITES, 5, **kw)
                    res, st = eng.partners(5, **kw)
                    for got, ref in zip((res["rows"], res["partner"], res["value_micro"]), want):
                        assert got.tobytes() == ref.tobytes(), (name, floor)
        finally:
            eng.close()
