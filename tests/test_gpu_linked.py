"""Linked pairs on the device (ngsld_linked_pairs, Engine.linked_pairs, the binary's --linked_* flags) against
tests/linked_ref.py -- the rule of LINKED.md in plain Python -- applied to the same engine's own full table (run_text).  The text
must be equal as bytes, and the records equal as bytes to the records Engine.run returns for those pairs: nothing sampled, no
tolerance.

The shapes are the smallest at which the kernels can still go wrong: rows longer than 64 candidates (a row spans items), row tails
shorter than 64, masks with holes (rnd_sample), more than one chromosome, chunks and slices that cut between the items of one
row -- 300 to 500 sites, 8 / 64 / 500 individuals, a 20 kb window over gaps of up to 300 bp, or all pairs at 300 sites.

GPU time of this file on one MI355X: see LINKED.md ("What the tests cost")."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import linked_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

KNOBS = ("NGSLD_TEST_LINKED_CHUNK_PAIRS", "NGSLD_TEST_LINKED_FORCE_HOST", "NGSLD_TEST_RECORD_SLICE_ITEMS")
INF = math.inf


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _labels(chrs, pos):
    return [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]


class Table:
    """The engine's own full output: the records of Engine.run and the table of run_text, row k of the one the pair k of the
    other.  Computed once per input and left unchanged."""

    def __init__(self, eng, labels):
        eng.set_text_output(None, False)
        self.s1, self.s2, self.std, self.ext = eng.run()
        eng.set_text_output(labels)
        text, fallbacks = eng.run_text()
        eng.set_text_output(None, False)
        assert fallbacks == 0
        self.text = text.decode()
        self.rows = self.text.splitlines()
        assert len(self.rows) == len(self.s1) > 0
        self.labels = labels
        self.label_cols = 1 if labels is None else labels[0].count("\t") + 1
        # the printed maf of every label, for a table without the extended columns
        self.maf = None if labels is None else {lab: float(f"{m:f}") for lab, m in zip(labels, eng.maf())}

    def want(self, **kw):
        """(indices of the linked rows, their text) by the rule."""
        mask = linked_ref.linked_mask(self.text, label_cols=self.label_cols, maf=self.maf, **kw)
        idx = np.flatnonzero(np.array(mask, dtype=bool))
        return idx, "".join(self.rows[k] + "\n" for k in idx).encode()


def _check(eng, tab, **kw):
    """Records + text, records only and text only: the rule's rows, as bytes; returns (result, stats)."""
    idx, text = tab.want(**kw)
    res, st = eng.linked_pairs(tab.labels, records=True, text=True, **kw)
    assert res["text"] == text, (len(res["text"]), len(text))
    assert res["s1"].dtype == np.uint32 and res["s2"].dtype == np.uint32
    assert res["s1"].tobytes() == tab.s1[idx].astype(np.uint32).tobytes()
    assert res["s2"].tobytes() == tab.s2[idx].astype(np.uint32).tobytes()
    assert res["std"].dtype == capi.REC_STD and res["std"].tobytes() == tab.std[idx].tobytes()
    if tab.ext is not None:
        assert res["ext"].dtype == capi.REC_EXT and res["ext"].tobytes() == tab.ext[idx].tobytes()
    else:
        assert "ext" not in res
    assert st["pairs"] == len(tab.rows) and st["rows"] == len(idx) and st["text_bytes"] == len(text)
    assert st["batches"] <= st["chunks"] and (st["batches"] > 0) == (len(idx) > 0)
    rec_only, st_r = eng.linked_pairs(tab.labels, records=True, text=False, **kw)
    assert "text" not in rec_only and st_r["text_bytes"] == 0 and st_r["host_rows"] == 0
    assert all(rec_only[k].tobytes() == res[k].tobytes() for k in rec_only) and set(rec_only) == set(res) - {"text"}
    text_only, st_t = eng.linked_pairs(tab.labels, records=False, text=True, **kw)
    assert set(text_only) == {"text"} and text_only["text"] == text and st_t["rows"] == len(idx)
    print(f"pairs {st['pairs']} rows {st['rows']} bytes {st['text_bytes']} host_rows {st['host_rows']} chunks {st['chunks']} pairs_ms "
          f"{st['pairs_ms']:.2f} kernel_ms {st['kernel_ms']:.3f} total_ms {st['total_ms']:.2f}")
    return res, st


WIN = dict(max_kb_dist=20, extend_out=True)
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, linked kw, geno kw)
    "n8_window": (500, 8, {}, 1, WIN, {}, None),
    "n64_window": (500, 64, {}, 1, WIN, {}, None),
    "n500_window": (400, 500, {}, 1, WIN, {}, None),
    "plain_columns": (500, 64, {}, 2, dict(max_kb_dist=20, extend_out=False), dict(min_weight=0.2), None),
    "r2_ExpG": (400, 64, {}, 1, WIN, dict(field=4, min_weight=0.3), None),
    "abs_D": (400, 64, {}, 1, WIN, dict(field=5, min_weight=0.05), None),
    "abs_Dp": (400, 64, {}, 1, WIN, dict(field=6, min_weight=0.9), None),
    "signed_D_negative_floor": (400, 64, {}, 1, WIN, dict(field=5, min_weight=-0.02, abs_value=False), None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=20, min_maf=0.1, rnd_sample=0.6, seed=7, extend_out=True),
                           dict(min_weight=0.2), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, dict(min_weight=0.1), None),
    "call_geno": (500, 64, {}, 1, WIN, dict(min_weight=0.3), dict(call_geno=(0.1, 0.9))),
    "max_snp_dist": (500, 64, {}, 2, dict(max_snp_dist=40, extend_out=True), dict(field=6, min_weight=0.8), None),
    "kb_limit_inside_the_window": (400, 64, {}, 1, WIN, dict(max_kb_dist=7.5, min_weight=0.1), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_linked_pairs_equal_the_rule_on_own_table(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n_sites, n_ind, skw, n_chr, plan_kw, kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 500 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 37, max_gap=300, n_chr=n_chr)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        row_off, _ = eng.plan_rows()
        assert int(np.diff(row_off).max()) > 64 or name == "max_snp_dist"  # (a row spans items; 40 candidates a row there)
        if name.endswith("_window"):  # (a one-slot group, an eight-slot group and the run kernel)
            want = {8: "group 1x1", 64: "group 1x8", 500: "run 1x8"}[n_ind]
            assert capi.describe_dispatch(n_ind).startswith(want) and eng.pair_kernel() == want.split()[0], capi.describe_dispatch(n_ind)
        tab = Table(eng, labels)
        res, st = _check(eng, tab, **kw)
        assert 0 < st["rows"] < st["pairs"] and st["chunks"] == 1 and st["host_rows"] == 0
        if name == "signed_D_negative_floor":
            d = res["std"]["D"]
            assert (d < 0).any() and (d > 0).any() and st["rows"] > _check(eng, tab, field=5, min_weight=0.02)[1]["rows"] // 2
        if name == "uncalled_mono":
            # nan / inf rows are in the table and never linked, whatever the floor; the replayed pairs carry their replayed digits:
            # the bytes are the table's own
            col = lambda f: 2 + linked_ref.FIELDS[f]  # noqa: E731
            bad = {f: sum(1 for r in tab.rows if not math.isfinite(float(r.split("\t")[col(f)]))) for f in (4, 5, 6, 7)}
            assert any(bad.values()), bad
            for f, n_bad in bad.items():
                if n_bad:
                    res_f, st_f = _check(eng, tab, field=f, min_weight=-INF, abs_value=False)
                    assert 0 < st_f["rows"] <= st["pairs"] - n_bad
                    assert all(math.isfinite(float(r.split(b"\t")[col(f)])) for r in res_f["text"].splitlines())
            print(f"non-finite rows by column {bad}, replayed pairs {eng.replay_info()['pairs_replayed']}")
        if name == "kb_limit_inside_the_window":
            assert st["rows"] < _check(eng, tab, min_weight=0.1)[1]["rows"]
        if name == "plain_columns":
            assert len(tab.rows[0].split("\t")) == 7 and len(set(chrs)) == 2
    finally:
        eng.close()


def _one_input(extra_label_col=False, labels_null=False, mono_frac=0.1):
    raw = synth.make_gl_numpy(500, 64, 71, depth=4.0, mono_frac=mono_frac)
    chrs, pos = synth.make_positions(500, 71, max_gap=300, n_chr=2)
    labels = None if labels_null else _labels(chrs, pos)
    if extra_label_col:
        labels = [f"{lab}\tsnp{k}" for k, lab in enumerate(labels)]
    return raw, chrs, pos, labels


def test_every_finite_row_at_minus_inf_and_no_row_above_every_value(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels = _one_input()
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, labels)
        for field in (5, 6, 7):
            res, st = _check(eng, tab, field=field, min_weight=-INF, abs_value=False)
            col = 2 + linked_ref.FIELDS[field]
            finite = [r for r in tab.rows if math.isfinite(float(r.split("\t")[col]))]
            # (the maf filter at its default never drops a row of a finite value here; D is finite in every row, D' and r2 are
            # nan in the rows of the monomorphic sites)
            assert res["text"] == "".join(r + "\n" for r in finite).encode()
            assert 0 < len(finite) < len(tab.rows) if field != 5 else len(finite) == len(tab.rows)
        # a floor above every value: no row, and the sink is never called
        calls = []
        res, st = eng.linked_pairs(labels, min_weight=1e9, records=True, text=True, on_batch=lambda k: calls.append(k) or 0)
        assert st["rows"] == 0 and st["batches"] == 0 and calls == [] and res["text"] == b"" and len(res["s1"]) == 0
        assert len(res["std"]) == 0 and len(res["ext"]) == 0 and st["chunks"] == 1 and st["pairs"] == len(tab.rows)
        _check(eng, tab, min_weight=INF)
    finally:
        eng.close()


def test_pass_min_maf_at_equality(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels = _one_input()
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, labels)
        printed = sorted(m for m in tab.maf.values() if not math.isnan(m))
        m = printed[len(printed) // 3]  # a value a site's maf prints: the comparison is exercised at equality
        assert f"\t{m:f}\t" in tab.text
        _, at = _check(eng, tab, min_weight=0.0, min_maf=m)
        _, above = _check(eng, tab, min_weight=0.0, min_maf=m + 1e-6)
        _, none = _check(eng, tab, min_weight=0.0)
        assert 0 < above["rows"] < at["rows"] < none["rows"]
    finally:
        eng.close()


def test_two_chromosomes_all_pairs_and_the_limit(monkeypatch):
    """max_kb_dist=0 in the plan: all pairs, the rows across the two chromosomes among them (dist inf).  At the default limit they
    are linked rows if their value is; with a finite limit, however large, they are gone."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw = synth.make_gl_numpy(300, 64, 864, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, dict(extend_out=True))
    try:
        tab = Table(eng, labels)
        assert len(tab.rows) == 300 * 299 // 2
        res, st = _check(eng, tab, min_weight=0.02)
        cross = int(np.count_nonzero((res["s1"] < 150) & (res["s2"] >= 150)))
        assert cross > 0 and b"\tinf\t" in res["text"]
        res2, st2 = _check(eng, tab, min_weight=0.02, max_kb_dist=1e6)
        assert st2["rows"] == st["rows"] - cross and b"\tinf\t" not in res2["text"]
        assert not ((res2["s1"] < 150) & (res2["s2"] >= 150)).any()
    finally:
        eng.close()


@pytest.mark.parametrize("how", ["null", "extra_column"])
def test_labels_null_and_with_an_extra_column(how, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels = _one_input(extra_label_col=how == "extra_column", labels_null=how == "null")
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, labels)
        res, st = _check(eng, tab, min_weight=0.2)
        first = res["text"].split(b"\n")[0].split(b"\t")
        if how == "null":
            assert first[:2] == [b"(null)", b"(null)"]
        else:
            assert first[1].startswith(b"snp") and first[3].startswith(b"snp") and tab.label_cols == 2
        assert st["rows"] > 0
    finally:
        eng.close()


def _chunks(row_off, chunk_pairs):
    """RecordPass's greedy rule, restated from plan_rows() as tests/test_gpu_grid.py does: consecutive rows while their pairs fit
    chunk_pairs, a row never cut; [(r0, r1, pairs)] of the chunks with pairs."""
    n, out, r = len(row_off) - 1, [], 0
    while r < n:
        e = r + 1
        while e < n and row_off[e + 1] - row_off[r] <= chunk_pairs:
            e += 1
        if row_off[e] > row_off[r]:
            out.append((r, e, int(row_off[e] - row_off[r])))
        r = e
    return out


def test_chunks_slices_and_the_host_formatter_give_the_same_bytes(monkeypatch):
    """Chunks of a tenth of the pairs and of one row each, slices of 64 and 7 items (a chunk in more than three launches, a slice
    beginning inside a row), every chunk through the host formatter: the one-chunk bytes."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels = _one_input()
    plan_kw = dict(max_kb_dist=20, extend_out=True, rnd_sample=0.8, seed=3)
    kw = dict(min_weight=0.1)
    eng = _engine(raw, chrs, pos, plan_kw)
    try:
        tab = Table(eng, labels)
        row_off = [int(x) for x in eng.plan_rows()[0]]
        n_pairs = row_off[-1]
        items = eng.items()
        base, st0 = _check(eng, tab, **kw)
        assert st0["chunks"] == 1 and st0["batches"] == 1 and st0["rows"] > 1000 and len(items) > 3 * 64
        tenth = n_pairs // 10
        runs = {
            "tenth": {"NGSLD_TEST_LINKED_CHUNK_PAIRS": str(tenth)},
            "row": {"NGSLD_TEST_LINKED_CHUNK_PAIRS": "1"},
            "slice64": {"NGSLD_TEST_RECORD_SLICE_ITEMS": "64"},
            "slice7": {"NGSLD_TEST_RECORD_SLICE_ITEMS": "7"},
            "tenth_slice7": {"NGSLD_TEST_LINKED_CHUNK_PAIRS": str(tenth), "NGSLD_TEST_RECORD_SLICE_ITEMS": "7"},
            "host": {"NGSLD_TEST_LINKED_FORCE_HOST": "1"},
            "host_tenth_slice7": {"NGSLD_TEST_LINKED_FORCE_HOST": "1", "NGSLD_TEST_LINKED_CHUNK_PAIRS": str(tenth),
                                  "NGSLD_TEST_RECORD_SLICE_ITEMS": "7"},
        }
        for name, env in runs.items():
            for k in KNOBS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            res, st = _check(eng, tab, **kw)
            assert all(res[k].tobytes() == base[k].tobytes() for k in ("s1", "s2", "std", "ext")) and res["text"] == base["text"], name
            chunk = int(env.get("NGSLD_TEST_LINKED_CHUNK_PAIRS", n_pairs))
            want = _chunks(row_off, chunk)
            assert st["chunks"] == len(want), (name, st["chunks"], len(want))
            if name == "tenth":
                assert len(want) > 10
            if name == "row":
                assert len(want) == sum(1 for a, b in zip(row_off, row_off[1:]) if b > a) > 400
            assert st["host_rows"] == (st["rows"] if "NGSLD_TEST_LINKED_FORCE_HOST" in env else 0), name
            # a sink called per chunk with rows, in order: never more often than there are chunks
            assert 1 <= st["batches"] <= st["chunks"]
        assert len(items) > 3 * 64  # (slices of 64 items cut the one chunk into more than three launches)
    finally:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        eng.close()


def test_a_sink_that_fails_on_its_second_call(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw, chrs, pos, labels = _one_input()
    eng = _engine(raw, chrs, pos, WIN)
    try:
        tab = Table(eng, labels)
        monkeypatch.setenv("NGSLD_TEST_LINKED_CHUNK_PAIRS", str(len(tab.rows) // 10))
        seen = []
        with pytest.raises(capi.NgsldError) as e:
            eng.linked_pairs(labels, min_weight=0.1, text=True, on_batch=lambda k: seen.append(k) or (7 if k == 2 else 0))
        assert e.value.code == 7 and seen == [1, 2] and "sink" in e.value.msg
        _, st = _check(eng, tab, min_weight=0.1)  # the context stays usable: the full result
        assert st["batches"] > 5
    finally:
        eng.close()


def test_rows_are_the_clusters_edges(monkeypatch):
    """One chromosome, integer gaps, a finite limit larger than the chromosome: the linked rows are exactly the edges of
    ngsld_clusters at the same field, floor and maf."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw = synth.make_gl_numpy(500, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 71, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        for kw in (dict(field=7, min_weight=0.2, min_maf=0.05), dict(field=5, min_weight=0.03, abs_value=False, min_maf=0.0)):
            _, st = eng.linked_pairs(None, max_kb_dist=1e6, records=True, **kw)
            _, table, cst = eng.clusters(max_kb_dist=1e6, min_size=1, **kw)
            assert st["rows"] == int(table["edges"].sum()) == cst["edges"] > 0
    finally:
        eng.close()


def test_refusals(monkeypatch, tmp_path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    raw = synth.make_gl_numpy(300, 16, 3, depth=4.0)
    chrs, pos = synth.make_positions(300, 37, max_gap=300)
    labels = _labels(chrs, pos)
    U, I = capi.ERR_UNSUPPORTED, capi.ERR_INVALID

    def refused(eng, code, *words, **kw):
        with pytest.raises(capi.NgsldError) as e:
            eng.linked_pairs(labels, **kw)
        assert e.value.code == code and all(w in e.value.msg for w in words), (e.value.code, e.value.msg)

    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        refused(eng, I, "ngsld_plan has not been called")
        eng.plan(**WIN)
        for f in (3, 8, 0, -1):
            refused(eng, I, "field must be a TSV column 4..7", field=f)
        refused(eng, I, "min_weight is NaN", min_weight=math.nan)
        refused(eng, I, "max_kb_dist", max_kb_dist=math.nan)
        refused(eng, I, "max_kb_dist", max_kb_dist=-1.0)
        refused(eng, I, "min_maf is NaN", min_maf=math.nan)
        refused(eng, I, "min_maf", min_maf=-0.1)
        refused(eng, I, "min_maf", min_maf=INF)
        refused(eng, I, "want", records=False, text=False)
        import ctypes as C
        p = capi.LinkedParams(C.sizeof(capi.LinkedParams) - 8, 7, 0.5, INF, 0.0, 1, 1)
        cb = capi.LINKED_FN(lambda _u, _b: 0)
        assert eng._L.ngsld_linked_pairs(eng._h, C.byref(p), None, cb, None, None) == I and b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = capi.LinkedParams(C.sizeof(capi.LinkedParams), 7, 0.5, INF, 0.0, 1, 1)
        st = capi.LinkedStats()  # (struct_size not set)
        assert eng._L.ngsld_linked_pairs(eng._h, C.byref(p), None, cb, None, C.byref(st)) == I
        assert eng._L.ngsld_linked_pairs(eng._h, C.byref(p), None, cb, None, None) == capi.OK  # (stats may be NULL)
        assert eng.linked_pairs(labels)[1]["rows"] > 0  # (a refusal leaves the context usable)
        # positions no file holds: half a base between sites.  A finite limit is refused; without one the call goes through, its
        # text from the host formatter, which adds the gaps one by one as the full table's writer does
        eng.set_pos_dist(np.full(300, 10.5))
        eng.plan(max_kb_dist=1, extend_out=True)
        refused(eng, U, "linked max_kb_dist needs integer position gaps", max_kb_dist=0.5)
        res, st = eng.linked_pairs(None, min_weight=0.1, text=True)
        assert st["rows"] > 0 and st["host_rows"] == st["rows"]
        eng.set_text_output(None, False)
        with open(tmp_path / "host_table.tsv", "wb") as fh:  # (the full table from the host writer, "(null)" labels)
            eng.run_to_fd(0, 300, fh.fileno(), None, np.full(300, 10.5), eng.maf(), 1)
        table = open(tmp_path / "host_table.tsv").read()
        assert len(table.splitlines()) == st["pairs"]
        assert res["text"] == linked_ref.linked(table, min_weight=0.1).encode()
    finally:
        eng.close()


# ---- ties: the reference program's table ----
def test_floor_on_a_printed_tie_of_the_reference_table(tmp_path, monkeypatch):
    """The tie-heavy input of tests/test_gpu_ties.py: 300 sites, called genotypes of 8 and 16 individuals, all pairs, D.  The floor
    on a value a tie prints and on the value the other rounding would print; expected = the rule over the REFERENCE program's
    table (which a wrong device value could not bend), its rows put in the table's order (the program's threads print as they
    finish).  The table has rows exactly on each floor."""
    import test_gpu_ties as ties
    if not ties.have_ref_program():
        pytest.skip("oracle/_ref predates ref_main (rebuild with oracle/build_ref.sh)")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for name in ("called_n8", "called_n16"):
        d = str(tmp_path / name)
        os.makedirs(d)
        case = ties.Case(name, d)
        text = ties._ref_table(case, True, d)
        rows = ties._ref_rows(case, text)
        index = {lab: k for k, lab in enumerate(case.labels)}
        eng = case.engine()
        try:
            eng.plan(extend_out=True)
            for q, up in ties._floors(case):
                assert ties._on(rows, q) > 0  # rows exactly on the floor
                counts = []
                for floor in (q, ties._other(q, up)):
                    lines = linked_ref.linked_lines(text, field=5, min_weight=floor / 10 ** 6)
                    lines.sort(key=lambda ln: tuple(index[x] for x in ln.split("\t")[:2]))
                    want = "".join(ln + "\n" for ln in lines).encode()
                    res, st = eng.linked_pairs(case.labels, field=5, min_weight=floor / 10 ** 6, records=True, text=True)
                    assert res["text"] == want, (name, floor)
                    assert [index[ln.split("\t")[0]] for ln in lines] == res["s1"].tolist()
                    counts.append(st["rows"])
                # rounded down: the other neighbour lies above and the boundary rows leave; rounded up: it lies below, they stay
                assert (counts[1] - counts[0] == ties._on(rows, q - 1)) if up else (counts[0] - counts[1] == ties._on(rows, q))
        finally:
            eng.close()


# ---- the binary ----
def test_cli_linked_out(tmp_path):
    n_sites, n_ind = 400, 64
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
    # next to --out in one run, beside another analysis: the linked file is the rule over that run's table
    r = run("--out", "t.tsv", "--linked_out", "l.tsv", "--linked_min_weight", "0.2", "--site_out", "u.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "==> Linked pairs:" in r.stderr
    table = open(tmp_path / "t.tsv").read()
    assert table.startswith("site1\t") and len(table) > 100_000
    want = linked_ref.linked(table, min_weight=0.2)
    assert 100 < len(want.splitlines()) < len(table.splitlines()) and open(tmp_path / "l.tsv").read() == want
    assert os.path.getsize(tmp_path / "u.tsv") > 0
    # alone: no TSV (not even on standard output); under the header, compressed; the other flags
    r = run("--linked_outH", "lh.tsv.gz", "--linked_field", "5", "--linked_signed", "--linked_min_weight=-0.01", "--linked_max_kb_dist", "7.5",
            "--linked_min_maf", "0.05")
    assert r.returncode == 0 and r.stdout == "", r.stderr[-2000:]
    want = linked_ref.linked(table, header=True, field=5, abs_value=False, min_weight=-0.01, max_kb_dist=7.5, min_maf=0.05)
    assert gzip.open(tmp_path / "lh.tsv.gz", "rt").read() == want and len(want.splitlines()) > 100
    r = run("--linked_out", "l2.tsv.gz", "--linked_field", "6", "--linked_min_weight", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert gzip.open(tmp_path / "l2.tsv.gz", "rt").read() == linked_ref.linked(table, field=6, min_weight=1.0)
    # a floor above every value: only the header, or nothing
    r = run("--linked_outH", "lh0.tsv", "--linked_min_weight", "1e9")
    assert r.returncode == 0 and open(tmp_path / "lh0.tsv").read() == table.split("\n", 1)[0] + "\n", r.stderr[-2000:]
    r = run("--linked_out", "l0.tsv", "--linked_min_weight", "inf")
    assert r.returncode == 0 and os.path.getsize(tmp_path / "l0.tsv") == 0, r.stderr[-2000:]
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--linked_out", "l5.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--linked_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "l5.tsv")
