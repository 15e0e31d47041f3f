"""The LD tree on the device (ngsld_ld_tree, Engine.ld_tree, Engine.ld_tree_cut, the binary's --tree_* flags) against
tests/tree_ref.py -- rules 2 to 5 of TREE.md in plain Python: sorted, a dictionary union-find -- applied to the same engine's own
TSV (run_text).  Every integer of the merges must be equal, and every cut must be, as bytes, what Engine.clusters gives at that
floor: nothing sampled, no tolerance.

A cut shows something only if it is neither one cluster nor all singletons: the floors of a case are the first three at which
the cut holds, on the engine's TSV, at least three clusters of three sites or more and at least one singleton
(test_gpu_clusters._floor's condition), and the case fails if there are fewer than three.  They are looked for in
test_gpu_clusters.FLOORS, in its order, and then -- single linkage chains 500 individuals' r2 into one cluster below 0.8 and
leaves only singletons from 0.99 on, so that FLOORS has two such floors there -- in the hundredths 0.01 ... 0.99 it does not hold.

GPU time of this file on one MI355X: see TREE.md ("What the tests cost")."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
import tree_ref
from ngsld_amd import capi, synth
from test_gpu_clusters import CASES, FLOORS, WIN, _engine, _labels, _tsv
from util import have_ref_program

pytestmark = pytest.mark.gpu

KNOB, SLICES, PLANT = "NGSLD_TEST_TREE_CHUNK_PAIRS", "NGSLD_TEST_RECORD_SLICE_ITEMS", "NGSLD_TEST_TREE_PLANT"
KEYS = ("s1", "s2", "q", "dist", "left", "right", "size", "first", "last")


def _same(merges, want):
    assert set(merges) == set(KEYS)
    for k in KEYS:
        assert [int(x) for x in merges[k]] == [r[k] for r in want], k


def _bytes(merges):
    return {k: merges[k].tobytes() for k in KEYS}


def _three_floors(nodes, rows, n_sites):
    """The first three floors of FLOORS, then of the other hundredths, whose cut is not trivial (rows: the merges at the lowest
    floor of FLOORS)."""
    got, seen = [], []
    for w in [*FLOORS, *(k / 100 for k in range(1, 100) if k / 100 not in FLOORS)]:
        sizes = np.bincount(np.array(tree_ref.cut(nodes, rows, n_sites, w)))[1:]
        big, single = int((sizes >= 3).sum()), int((sizes == 1).sum())
        seen.append((w, big, single))
        if big >= 3 and single >= 1:
            got.append(w)
            if len(got) == 3:
                return got
    pytest.fail(f"fewer than three floors give three clusters of three sites and a singleton: (floor, clusters >= 3, singletons) {seen}")


@pytest.mark.parametrize("name", list(CASES))
def test_tree_equals_the_rule_on_own_tsv_and_its_cuts_the_clusters(name):
    n_sites, n_ind, skw, n_chr, plan_kw, kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 700 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 41, max_gap=300, n_chr=n_chr)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, labels)
        low_nodes, low_rows = tree_ref.tree(text, labels, **{**kw, "min_weight": min(FLOORS)})
        floors = _three_floors(low_nodes, low_rows, n_sites)
        base = min(floors)
        merges, stats = eng.ld_tree(min_weight=base, **kw)
        nodes, want = tree_ref.tree(text, labels, **{**kw, "min_weight": base})
        print(f"floors {floors} pairs {stats['pairs']} nodes {stats['nodes']} edges {stats['edges']} merges {stats['merges']} clusters "
              f"{stats['clusters']} chunks {stats['chunks']} rounds {stats['rounds']} pairs_ms {stats['pairs_ms']:.2f} edges_ms "
              f"{stats['edges_ms']:.3f} reduce_ms {stats['reduce_ms']:.3f} finish_ms {stats['finish_ms']:.3f} total_ms {stats['total_ms']:.2f}")
        _same(merges, want)
        _, edges = cluster_ref.tsv_edges(text, labels, **{**kw, "min_weight": base})
        assert stats["pairs"] == sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))
        assert stats["nodes"] == len(nodes) and stats["edges"] == len(edges) and stats["merges"] == len(want) > 0
        assert stats["merges"] == stats["nodes"] - stats["clusters"]
        assert stats["chunks"] == 1 and stats["displaced"] == 0 and 1 <= stats["max_rounds"] <= math.ceil(math.log2(n_sites)) + 1
        for t in floors:
            ids = eng.ld_tree_cut(t)
            cl_ids, _, cl_stats = eng.clusters(min_weight=t, min_size=1, **kw)
            assert ids.dtype == cl_ids.dtype and ids.tobytes() == cl_ids.tobytes(), t
            assert [int(x) for x in ids] == tree_ref.cut(nodes, want, n_sites, t), t
            n_cl = C.c_uint64(0)
            assert eng._L.ngsld_ld_tree_cut(eng._h, t, None, C.byref(n_cl)) == capi.OK and n_cl.value == cl_stats["clusters"]
        # the clusters calls in between took nothing from the tree
        again, _ = eng.ld_tree(min_weight=base, **kw)
        assert _bytes(again) == _bytes(merges)
        # fewer rows than merges: the arrays are filled up to cap, *n is the number there is
        q2, n = np.zeros(2, dtype=np.int64), C.c_uint64(0)
        assert eng._L.ngsld_ld_tree_merges(eng._h, 2, None, None, q2.ctypes.data, None, None, None, None, None, None, C.byref(n)) == capi.OK
        assert n.value == len(want) > 2 and q2.tolist() == [r["q"] for r in want[:2]]
    finally:
        eng.close()


# ---- ties ----
def _other_way(edges):
    """The forest when equal weights go the other way round: s2 descending first."""
    parent, kept = {}, set()
    for e in sorted(edges, key=lambda e: (-e[2], -e[1], -e[0])):
        parent.setdefault(e[0], e[0])
        parent.setdefault(e[1], e[1])
        a, b = tree_ref._find(parent, e[0]), tree_ref._find(parent, e[1])
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.add(e)
    return kept


@pytest.mark.parametrize("name", ["called_n8", "call_geno_n8"])
def test_equal_weights_go_by_the_rule(name, tmp_path):
    """Called genotypes of 8 individuals, all pairs of 300 sites: a few hundred distinct r2 over 44,850 pairs, so that most edges of
    the forest have rivals of their own weight, and the forest changes when the ties go another way.  Held to the rule on the
    engine's table and, where the reference program is built, on that program's own table."""
    from test_gpu_ties import Case, _ref_table
    case = Case(name, str(tmp_path))
    eng = case.engine()
    try:
        eng.plan(extend_out=True)
        text = _tsv(eng, case.labels)
        merges, stats = eng.ld_tree(min_weight=0.0)
    finally:
        eng.close()
    nodes, want = tree_ref.tree(text, case.labels, min_weight=0.0)
    _, edges = cluster_ref.tsv_edges(text, case.labels, min_weight=0.0)
    rule = {(r["s1"], r["s2"], r["q"]) for r in want}
    changed = len(rule - _other_way(edges))
    distinct = len({r["q"] for r in want})
    print(f"{name}: {len(want)} merges over {distinct} distinct printed values, {changed} change when ties go the other way round; "
          f"edges {stats['edges']} rounds {stats['rounds']}")
    assert len(want) >= 100 and distinct < len(want) and changed >= 50
    _same(merges, want)
    assert stats["merges"] == stats["nodes"] - stats["clusters"] == len(want)
    if have_ref_program():
        ref_text = _ref_table(case, True, str(tmp_path))
        _same(merges, tree_ref.tree(ref_text, case.labels, min_weight=0.0)[1])


# ---- chunks ----
@pytest.mark.parametrize("slices", [False, True])
@pytest.mark.parametrize("floor", [0.0, 0.1])
@pytest.mark.parametrize("name", ["n64_window", "n500_window"])
def test_small_chunks_give_the_same_bytes_and_replace_forest_edges(name, floor, slices, monkeypatch):
    n_sites, n_ind, skw, n_chr, plan_kw, kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 700 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 41, max_gap=300, n_chr=n_chr)
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv(SLICES, raising=False)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        one, s_one = eng.ld_tree(min_weight=floor)
        assert s_one["chunks"] == 1 and s_one["displaced"] == 0 and s_one["merges"] > 100
        monkeypatch.setenv(KNOB, "5000")
        if slices:
            monkeypatch.setenv(SLICES, "7")
        cut, s_cut = eng.ld_tree(min_weight=floor)
    finally:
        eng.close()
    print(f"{name} floor {floor} slices {slices}: chunks {s_cut['chunks']} displaced {s_cut['displaced']} rounds {s_cut['rounds']} "
          f"max_rounds {s_cut['max_rounds']} edges {s_cut['edges']} merges {s_cut['merges']} reduce_ms {s_cut['reduce_ms']:.2f}")
    assert _bytes(cut) == _bytes(one)
    assert s_cut["chunks"] >= 10 and s_cut["displaced"] > 0
    assert all(s_cut[k] == s_one[k] for k in ("pairs", "nodes", "edges", "merges", "clusters"))
    assert s_cut["max_rounds"] <= math.ceil(math.log2(n_sites)) + 1


# ---- depth ----
def test_a_path_of_twenty_thousand_sites_takes_sixteen_rounds_at_most(monkeypatch):
    """max_snp_dist 1 emits only adjacent pairs and at min_weight 0 every finite one is an edge: the graph is a path and the
    forest is the graph.  The rounds of a reduce are bounded by the logarithm of the sites, not by the path's length."""
    n = 20000
    monkeypatch.delenv(KNOB, raising=False)
    raw = synth.make_gl_numpy(n, 64, 20064, depth=4.0)
    chrs, pos = synth.make_positions(n, 43, max_gap=300)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, dict(max_snp_dist=1, extend_out=True))
    try:
        text = _tsv(eng, labels)
        one, s_one = eng.ld_tree(min_weight=0.0)
        monkeypatch.setenv(KNOB, "1000")
        cut, s_cut = eng.ld_tree(min_weight=0.0)
    finally:
        eng.close()
    print(f"one chunk: rounds {s_one['rounds']} reduce_ms {s_one['reduce_ms']:.2f}; {s_cut['chunks']} chunks: rounds {s_cut['rounds']} "
          f"max_rounds {s_cut['max_rounds']} reduce_ms {s_cut['reduce_ms']:.2f}")
    assert s_one["merges"] == s_one["edges"] == n - 1 and s_one["chunks"] == 1
    assert s_one["max_rounds"] <= 16 and s_cut["max_rounds"] <= 16  # (ceil(log2(20,000)) + 1)
    assert s_cut["chunks"] >= 19 and _bytes(cut) == _bytes(one)
    _same(one, tree_ref.tree(text, labels, min_weight=0.0)[1])


# ---- refusals ----
def _small():
    raw = synth.make_gl_numpy(500, 64, 91, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 91, max_gap=300)
    return raw, chrs, pos


def _no_tree(eng):
    n = C.c_uint64(0)
    assert eng._L.ngsld_ld_tree_merges(eng._h, 0, None, None, None, None, None, None, None, None, None, C.byref(n)) == capi.ERR_INVALID
    assert b"no ngsld_ld_tree result" in eng._L.ngsld_last_error(eng._h)
    with pytest.raises(capi.NgsldError) as e:
        eng.ld_tree_cut(0.5)
    assert e.value.code == capi.ERR_INVALID and "no ngsld_ld_tree result" in e.value.msg


@pytest.mark.parametrize("cut", [False, True])
def test_a_planted_value_of_2_38_micro_units_is_refused_naming_the_pair(cut, monkeypatch):
    """No input gives a finite value near 274877.906944, so NGSLD_TEST_TREE_PLANT writes one into the record of one pair before the
    candidates kernel reads it.  2^38 micro-units, of either sign, are refused naming the pair and leave no tree; 2^38 - 1 are the
    first merge."""
    raw, chrs, pos = _small()
    labels = _labels(chrs, pos)
    for k in (KNOB, SLICES, PLANT):
        monkeypatch.delenv(k, raising=False)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        lines = [ln for ln in _tsv(eng, labels).splitlines() if ln and not ln.startswith("site1\t")]
        at = next(k for k in range(2 * len(lines) // 3, len(lines))
                  if (lambda g: labels.index(g[1]) > labels.index(g[0]) + 1 and math.isfinite(float(g[6])))(lines[k].split("\t")))
        i, j = (labels.index(x) for x in lines[at].split("\t")[:2])
        if cut:
            monkeypatch.setenv(KNOB, str(len(lines) // 10))
            monkeypatch.setenv(SLICES, "7")
        base, st = eng.ld_tree()
        assert (st["chunks"] > 1) == cut
        for value in ("274877.906944", "-274877.906944", "1e300"):
            monkeypatch.setenv(PLANT, f"{at}:{value}")
            with pytest.raises(capi.NgsldError) as e:
                eng.ld_tree()
            assert e.value.code == capi.ERR_UNSUPPORTED, e.value.msg
            assert f"a tree value of the pair of sites {i} - {j} reaches 2^38 micro-units" in e.value.msg, e.value.msg
            _no_tree(eng)
        monkeypatch.setenv(PLANT, f"{at}:-274877.906943")
        top, _ = eng.ld_tree()
        assert (int(top["s1"][0]), int(top["s2"][0]), int(top["q"][0])) == (i, j, 2 ** 38 - 1)
        _, s_abs = eng.ld_tree(min_weight=1.0)
        _, s_signed = eng.ld_tree(min_weight=1.0, abs_value=False)  # (signed, the planted value is below every floor)
        assert s_abs["edges"] == s_signed["edges"] + 1
        monkeypatch.delenv(PLANT)
        again, _ = eng.ld_tree()
    finally:
        eng.close()
    assert _bytes(again) == _bytes(base)


def test_refusals_leave_no_tree_and_a_usable_context():
    raw = synth.make_gl_numpy(100, 16, 3, depth=4.0)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(np.full(100, 10.0))
        eng.plan(max_kb_dist=1, extend_out=True)
        _no_tree(eng)  # before any tree
        merges, st = eng.ld_tree(min_weight=0.2)
        assert st["nodes"] == 100 and st["merges"] == len(merges["q"]) > 0
        # a cut below the floor, or at no number: refused with a message, and the tree stays
        for t in (0.19, -1.0, math.nan):
            with pytest.raises(capi.NgsldError) as e:
                eng.ld_tree_cut(t)
            assert e.value.code == capi.ERR_INVALID and "min_weight" in e.value.msg, e.value.msg
        at_floor = eng.ld_tree_cut(0.2)
        assert int(at_floor.max()) == st["clusters"] and (eng.ld_tree_cut(math.inf) == np.arange(1, 101)).all()
        # parameters: refused before anything runs, the last tree stays
        P, S = capi.TreeParams, capi.TreeStats
        p = P(C.sizeof(P) - 8, 7, math.inf, 0.0, 0.1, 1, 0)
        assert eng._L.ngsld_ld_tree(eng._h, C.byref(p), None) == capi.ERR_INVALID
        assert b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = P(C.sizeof(P), 7, math.inf, 0.0, 0.1, 1, 0)
        assert eng._L.ngsld_ld_tree(eng._h, C.byref(p), C.byref(S())) == capi.ERR_INVALID  # (struct_size not set)
        for field in (3, 8):
            p.field = field
            assert eng._L.ngsld_ld_tree(eng._h, C.byref(p), None) == capi.ERR_INVALID
        p.field, p.min_weight = 7, math.nan
        assert eng._L.ngsld_ld_tree(eng._h, C.byref(p), None) == capi.ERR_INVALID
        assert eng.ld_tree_cut(0.2).tobytes() == at_floor.tobytes()
        # a new plan takes the tree with it
        eng.plan(max_kb_dist=1, extend_out=True)
        _no_tree(eng)
        # positions no file holds -- half a base between sites: refused, no tree, and the context goes on
        eng.ld_tree(min_weight=0.2)
        eng.set_pos_dist(np.full(100, 10.5))
        eng.plan(max_kb_dist=1, extend_out=True)
        with pytest.raises(capi.NgsldError) as e:
            eng.ld_tree()
        assert e.value.code == capi.ERR_UNSUPPORTED and "integer position gaps" in e.value.msg
        _no_tree(eng)
        eng.set_pos_dist(np.full(100, 10.0))
        eng.plan(max_kb_dist=1, extend_out=True)
        back, _ = eng.ld_tree(min_weight=0.2)
        assert _bytes(back) == _bytes(merges)
    finally:
        eng.close()


# ---- the binary ----
def test_cli_tree_files(tmp_path):
    n_sites, n_ind = 500, 64
    raw = synth.make_gl_numpy(n_sites, n_ind, 97, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 97, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "20",
            "--extend_out"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("NGSLD_TEST_")}
    run = lambda *a, env=env: subprocess.run([*base, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=300,  # noqa: E731
                                             env=env)
    r = run("--out", "t0.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    table = open(tmp_path / "t0.tsv").read()
    kw = dict(min_maf=0.05, max_kb_dist=15.0)
    tk = ["--tree_min_weight", "0.2", "--tree_min_maf", "0.05", "--tree_max_kb_dist", "15"]
    floors = ["0.8", "0.5", ".2"]
    # the two files alone: no TSV (not even on standard output)
    r = run("--tree_out", "tree.tsv", "--tree_cut", ",".join(floors), "--tree_cut_out", "cuts.tsv", *tk)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> LD tree:" in r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".tsv")) == ["cuts.tsv", "t0.tsv", "tree.tsv"]
    nodes, rows = tree_ref.tree(table, labels, min_weight=0.2, **kw)
    assert len(rows) > 50
    assert open(tmp_path / "tree.tsv").read() == tree_ref.tree_file(rows, labels)
    columns = [tree_ref.cut(nodes, rows, n_sites, float(t)) for t in floors]
    assert open(tmp_path / "cuts.tsv").read() == tree_ref.cuts_file(columns, floors, labels)
    # the cut columns are --cluster_out of separate commands at those floors
    for t, col in zip(floors, columns):
        r = run("--cluster_out", "c.tsv", "--cluster_min_weight", t, "--cluster_min_maf", "0.05", "--cluster_max_kb_dist", "15")
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(tmp_path / "c.tsv").read() == cluster_ref.cluster_file(col, labels), t
    # beside the table and another analysis: the table's bytes are those of a run without the tree flags; signed D
    r = run("--out", "t.tsv", "--tree_out", "tree5.tsv", "--tree_field", "5", "--tree_signed", "--tree_min_weight", "0.02", "--site_out", "s.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "t.tsv").read() == table and os.path.getsize(tmp_path / "s.tsv") > 0
    rows5 = tree_ref.tree(table, labels, field=5, abs_value=False, min_weight=0.02)[1]
    assert len(rows5) > 50 and open(tmp_path / "tree5.tsv").read() == tree_ref.tree_file(rows5, labels)
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--tree_out", "tree6.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--tree_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "tree6.tsv")
