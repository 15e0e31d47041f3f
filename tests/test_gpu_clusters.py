"""LD clusters on the device (ngsld_clusters, Engine.clusters, the binary's --cluster_* flags) against tests/cluster_ref.py --
the rule of CLUSTERS.md in plain Python, a dictionary union-find -- applied to the same engine's own TSV (run_text).  Every
site's cluster id and every integer of the table must be equal, every mean and density bit for bit: nothing sampled, no
tolerance.

A case shows something only if its graph is neither one cluster nor all singletons: where a case does not name its floor, the
first of FLOORS at which the restatement finds, on the engine's TSV, at least three clusters of three sites or more and at
least one singleton is taken (and the case fails if there is none).

GPU time of this file on one MI355X: see CLUSTERS.md ("What the tests cost")."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu

FLOORS = (0.5, 0.4, 0.3, 0.2, 0.15, 0.1, 0.07, 0.05, 0.03, 0.02, 0.01, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.995, 0.999, 0.9999)
KNOB = "NGSLD_TEST_CLUSTER_CHUNK_PAIRS"


def _engine(raw, chrs, pos, plan_kw, geno_kw=None):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw, **(geno_kw or {}))
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    eng.plan(**plan_kw)
    return eng


def _labels(chrs, pos):
    return [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]


def _tsv(eng, labels):
    eng.set_text_output(labels)
    text, fallbacks = eng.run_text()
    assert fallbacks == 0
    return text.decode()


def _shape(table):
    return sum(1 for r in table if r["size"] >= 3), sum(1 for r in table if r["size"] == 1)


def _floor(text, labels, kw):
    """The first floor of FLOORS that makes the case non-trivial on this TSV."""
    seen = []
    for w in FLOORS:
        big, single = _shape(cluster_ref.clusters(text, labels, min_size=1, min_weight=w, **kw)[1])
        seen.append((w, big, single))
        if big >= 3 and single >= 1:
            return w
    pytest.fail(f"no floor gives three clusters of three sites and a singleton: (floor, clusters >= 3, singletons) {seen}")


def _bits(values):
    return [None if v is None or (isinstance(v, float) and math.isnan(v)) else np.float64(v).view(np.int64).item() for v in values]


def _same(ids, table, want_ids, want_table):
    assert [int(x) for x in ids] == want_ids
    assert set(table) == {"id", "size", "first", "last", "span", "edges", "sum", "mean", "density"}
    for k in ("id", "size", "first", "last", "span", "edges", "sum"):
        assert [int(x) for x in table[k]] == [r[k] for r in want_table], k
    for k in ("mean", "density"):
        assert _bits(float(x) for x in table[k]) == _bits(r[k] for r in want_table), k


def _case(raw, chrs, pos, plan_kw, kw, geno_kw=None, min_size=2):
    """Engine.clusters against cluster_ref over the engine's own TSV; returns (ids, table, stats, the TSV, the floor)."""
    labels = _labels(chrs, pos)
    kw = dict(kw)
    eng = _engine(raw, chrs, pos, plan_kw, geno_kw)
    try:
        text = _tsv(eng, labels)
        if "min_weight" not in kw:
            kw["min_weight"] = _floor(text, labels, kw)
        ids, table, stats = eng.clusters(min_size=min_size, **kw)
    finally:
        eng.close()
    want_ids, want_all = cluster_ref.clusters(text, labels, min_size=1, **kw)
    _same(ids, table, want_ids, [r for r in want_all if r["size"] >= min_size])
    assert stats["pairs"] == sum(1 for ln in text.splitlines() if ln and not ln.startswith("site1\t"))
    assert stats["nodes"] == sum(1 for k in want_ids if k) and stats["edges"] == sum(r["edges"] for r in want_all)
    assert stats["clusters"] == len(want_all) == max(want_ids, default=0)
    assert stats["clusters_multi"] == sum(1 for r in want_all if r["size"] >= 2)
    assert stats["largest"] == max((r["size"] for r in want_all), default=0)
    assert stats["union_launches"] == stats["chunks"]
    big, single = _shape(want_all)
    print(f"floor {kw['min_weight']} pairs {stats['pairs']} nodes {stats['nodes']} edges {stats['edges']} clusters {stats['clusters']} "
          f"(>= 3 sites: {big}, singletons: {single}, largest {stats['largest']}) chunks {stats['chunks']} pairs_ms {stats['pairs_ms']:.2f} "
          f"union_ms {stats['union_ms']:.3f} finish_ms {stats['finish_ms']:.3f} total_ms {stats['total_ms']:.2f}")
    return ids, table, stats, text, kw["min_weight"]


# extend_out everywhere: the restatement applies the maf filter where the TSV has maf1 / maf2
WIN = dict(max_kb_dist=20, extend_out=True)
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, clusters kw, geno kw)
    # (8 individuals: r2 is noise over a 20 kb window and joins everything below 0.99; 3 kb leaves structure)
    "n8_window": (500, 8, {}, 1, dict(max_kb_dist=3, extend_out=True), {}, None),
    "n64_window": (500, 64, {}, 1, WIN, {}, None),
    "n500_window": (400, 500, {}, 1, WIN, {}, None),
    "allpairs_two_chr": (300, 64, {}, 2, dict(extend_out=True), {}, None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=30, min_maf=0.1, rnd_sample=0.6, seed=7, extend_out=True),
                           dict(min_maf=0.15), None),
    "field4": (400, 64, {}, 1, WIN, dict(field=4), None),
    "field5": (400, 64, {}, 1, WIN, dict(field=5), None),
    "field6": (400, 64, {}, 1, dict(max_kb_dist=3, extend_out=True), dict(field=6), None),  # (D' is 1 for most distant pairs)
    "field7": (400, 64, {}, 1, WIN, dict(field=7), None),
    "signed_D": (400, 64, {}, 1, WIN, dict(field=5, abs_value=False), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, {}, None),
    "call_geno": (500, 64, {}, 1, WIN, {}, dict(call_geno=(0.1, 0.9))),
    "kb_limit_inside_the_window": (400, 64, {}, 1, WIN, dict(max_kb_dist=7.5), None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_clusters_equal_the_rule_on_own_tsv(name):
    n_sites, n_ind, skw, n_chr, plan_kw, kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 700 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 41, max_gap=300, n_chr=n_chr)
    ids, _, stats, text, _ = _case(raw, chrs, pos, plan_kw, kw, geno_kw)
    if name == "allpairs_two_chr":
        assert stats["pairs"] == 300 * 299 // 2
        assert not set(ids[:150][ids[:150] > 0]) & set(ids[150:][ids[150:] > 0])  # (no cluster crosses the chromosomes)
    if name == "signed_D":
        # (this generator's negative D stay above -0.15, short of any floor that leaves structure: at a floor below all of them
        # every finite pair is an edge -- one cluster per run of sites, which shows nothing about the union -- and the sum is
        # the signed one)
        assert any(ln.split("\t")[4].startswith("-0.") and float(ln.split("\t")[4]) < 0 for ln in text.splitlines())
        _, t_signed, s_signed, _, _ = _case(raw, chrs, pos, plan_kw, dict(field=5, abs_value=False, min_weight=-1.0), geno_kw)
        _, t_abs, s_abs, _, _ = _case(raw, chrs, pos, plan_kw, dict(field=5, min_weight=-1.0), geno_kw)
        assert s_signed["edges"] == s_abs["edges"] > 0 and int(t_signed["sum"].sum()) < int(t_abs["sum"].sum())


def test_min_size_one_lists_the_singletons_and_ids_do_not_depend_on_it():
    raw = synth.make_gl_numpy(500, 64, 81, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 81, max_gap=300)
    ids1, t1, s1, _, floor = _case(raw, chrs, pos, WIN, {}, min_size=1)
    ids3, t3, _, _, _ = _case(raw, chrs, pos, WIN, dict(min_weight=floor), min_size=3)
    assert ids1.tobytes() == ids3.tobytes() and len(t1["id"]) == s1["clusters"] > len(t3["id"]) >= 3
    assert np.isnan(t1["mean"][t1["size"] == 1]).all() and np.isnan(t1["density"][t1["size"] == 1]).all()
    assert set(t3["id"]) <= set(t1["id"]) and (t3["size"] >= 3).all()


def _knob_case(monkeypatch, value, floor=None):
    monkeypatch.delenv(KNOB, raising=False)
    if value is not None:
        monkeypatch.setenv(KNOB, value)
    raw = synth.make_gl_numpy(600, 64, 71, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(600, 71, max_gap=300)
    kw = {} if floor is None else dict(min_weight=floor)
    ids, table, stats, _, floor = _case(raw, chrs, pos, dict(max_kb_dist=30, extend_out=True), kw, min_size=1)
    return ids, table, stats, floor


def test_default_and_small_chunks_give_the_same_arrays(monkeypatch):
    ids0, t0, s0, floor = _knob_case(monkeypatch, None)
    assert s0["chunks"] == 1 and s0["clusters_multi"] >= 3
    ids1, t1, s1, _ = _knob_case(monkeypatch, "3000", floor)
    assert s1["chunks"] > 5
    ids2, t2, s2, _ = _knob_case(monkeypatch, "700", floor)
    assert s2["chunks"] > s1["chunks"]
    for ids, t in ((ids1, t1), (ids2, t2)):
        assert ids.tobytes() == ids0.tobytes() and t.keys() == t0.keys()
        for k in t0:
            assert t[k].tobytes() == t0[k].tobytes(), k


@pytest.mark.parametrize("chunk", [None, "1000"])
def test_paths_of_twenty_thousand_sites_take_a_launch_per_chunk(monkeypatch, chunk):
    """max_snp_dist 1 emits only adjacent pairs and at min_weight 0 every finite one is an edge: the components are paths, as long
    as monomorphic sites and the chromosome change leave them.  The restatement decides what they are; the union takes one
    launch per chunk, whatever the diameter."""
    monkeypatch.delenv(KNOB, raising=False)
    if chunk is not None:
        monkeypatch.setenv(KNOB, chunk)
    raw = synth.make_gl_numpy(20000, 64, 20064, depth=4.0)
    chrs, pos = synth.make_positions(20000, 43, max_gap=300, n_chr=2)
    _, _, stats, _, _ = _case(raw, chrs, pos, dict(max_snp_dist=1, extend_out=True), dict(min_weight=0.0), min_size=1)
    assert stats["pairs"] >= 19998 and stats["largest"] >= 256  # (paths far longer than a wavefront or a workgroup)
    assert stats["union_launches"] == stats["chunks"] and (stats["chunks"] == 1 if chunk is None else stats["chunks"] >= 19)


def test_against_pruning_every_cluster_keeps_a_site():
    """Same plan, same graph (field, min_weight, max_kb_dist, weight type a, no maf filter): the nodes are the same sites,
    remove-heaviest never empties a component, and a site without an edge is never removed."""
    raw = synth.make_gl_numpy(500, 64, 1064, depth=4.0)
    chrs, pos = synth.make_positions(500, 37, max_gap=300, n_chr=2)
    labels = _labels(chrs, pos)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        floor = _floor(_tsv(eng, labels), labels, dict(max_kb_dist=12.0))
        ids, table, st = eng.clusters(field=7, min_weight=floor, max_kb_dist=12.0, min_size=1)
        state, pst = eng.prune(labels, field=7, max_kb_dist=12.0, min_weight=floor, weight_type="a")
    finally:
        eng.close()
    assert np.array_equal(state != 0, ids != 0) and st["nodes"] == pst["nodes"] and st["edges"] == pst["edges"] > 0
    kept = np.zeros(st["clusters"] + 1, dtype=bool)
    kept[ids[state == 1]] = True
    assert kept[1:].all() and pst["kept"] >= st["clusters"] and pst["excluded"] > 0
    single = np.isin(ids, table["id"][table["size"] == 1])
    assert single.any() and (state[single] == 1).all()


def test_two_calls_give_the_same_bits_and_the_result_goes_with_the_plan():
    raw = synth.make_gl_numpy(500, 64, 91, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(500, 91, max_gap=300)
    eng = _engine(raw, chrs, pos, WIN)
    try:
        a_ids, a, sa = eng.clusters(min_weight=0.3, min_size=1)
        b_ids, b, sb = eng.clusters(min_weight=0.3, min_size=1)
        ids = np.zeros(500, dtype=np.uint32)
        n = C.c_uint64(0)
        assert eng._L.ngsld_clusters_sites(eng._h, ids.ctypes.data) == capi.OK and ids.tobytes() == a_ids.tobytes()
        # fewer rows than clusters: the arrays are filled up to cap, *n is the number there is
        first = np.zeros(2, dtype=np.uint32)
        assert eng._L.ngsld_clusters_table(eng._h, 1, 2, None, None, first.ctypes.data, None, None, None, None, None, None, C.byref(n)) == capi.OK
        assert n.value == sa["clusters"] > 2 and first.tolist() == a["first"][:2].tolist()
        eng.plan(**WIN)
        assert eng._L.ngsld_clusters_sites(eng._h, ids.ctypes.data) == capi.ERR_INVALID
        assert eng._L.ngsld_clusters_table(eng._h, 1, 0, None, None, None, None, None, None, None, None, None, C.byref(n)) == capi.ERR_INVALID
    finally:
        eng.close()
    assert sa["edges"] == sb["edges"] > 0 and a_ids.tobytes() == b_ids.tobytes()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals():
    raw = synth.make_gl_numpy(100, 16, 3, depth=4.0)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(np.full(100, 10.5))  # (positions no file holds: half a base between sites)
        eng.plan(max_kb_dist=1, extend_out=True)
        with pytest.raises(capi.NgsldError) as e:
            eng.clusters()
        assert e.value.code == capi.ERR_UNSUPPORTED and "integer position gaps" in e.value.msg
        eng.set_pos_dist(np.full(100, 10.0))
        eng.plan(max_kb_dist=1, extend_out=True)
        ids, _, st = eng.clusters(min_weight=0.0)
        assert st["nodes"] == 100 and (ids > 0).all()
        P, S = capi.ClustersParams, capi.ClustersStats
        p = P(C.sizeof(P) - 8, 7, math.inf, 0.0, 0.5, 1, 0)
        assert eng._L.ngsld_clusters(eng._h, C.byref(p), None) == capi.ERR_INVALID
        assert b"struct_size" in eng._L.ngsld_last_error(eng._h)
        p = P(C.sizeof(P), 7, math.inf, 0.0, 0.5, 1, 0)
        st = S()  # (struct_size not set)
        assert eng._L.ngsld_clusters(eng._h, C.byref(p), C.byref(st)) == capi.ERR_INVALID
        assert b"struct_size" in eng._L.ngsld_last_error(eng._h)
        for field in (3, 8):
            p.field = field
            assert eng._L.ngsld_clusters(eng._h, C.byref(p), None) == capi.ERR_INVALID
        p.field, p.min_weight = 7, math.nan
        assert eng._L.ngsld_clusters(eng._h, C.byref(p), None) == capi.ERR_INVALID
        # (a call refused for its parameters leaves the last result in place)
        assert eng._L.ngsld_clusters_sites(eng._h, ids.ctypes.data) == capi.OK and (ids > 0).all()
    finally:
        eng.close()


def test_cli_cluster_files(tmp_path):
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
    table = open(tmp_path / "t0.tsv", "rb").read()
    assert len(table) > 100_000
    ref_kw = dict(min_maf=0.05, max_kb_dist=15.0)
    floor = _floor(table.decode(), labels, ref_kw)
    ck = ["--cluster_min_weight", repr(floor), "--cluster_min_maf", "0.05", "--cluster_max_kb_dist", "15"]
    # the two files alone: no TSV (not even on standard output)
    r = run("--cluster_out", "c.tsv", "--cluster_table", "k.tsv", *ck)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == "" and "==> LD clusters:" in r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".tsv")) == ["c.tsv", "k.tsv", "t0.tsv"]
    # beside the table: its bytes are those of a run without the cluster flags
    r = run("--out", "t.tsv", "--cluster_table", "k1.tsv", "--cluster_min_size", "1", *ck)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "t.tsv", "rb").read() == table and not os.path.exists(tmp_path / "c1.tsv")
    ids, rows = cluster_ref.clusters(table.decode(), labels, min_size=1, min_weight=floor, **ref_kw)
    assert open(tmp_path / "c.tsv").read() == cluster_ref.cluster_file(ids, labels)
    assert open(tmp_path / "k.tsv").read() == cluster_ref.table_file([r for r in rows if r["size"] >= 2], labels)
    assert open(tmp_path / "k1.tsv").read() == cluster_ref.table_file(rows, labels)
    assert "\tNA\tNA\n" in open(tmp_path / "k1.tsv").read()
    # signed D, and beside the other analyses
    floor_d = _floor(table.decode(), labels, dict(field=5, abs_value=False))
    r = run("--cluster_out", "c3.tsv", "--cluster_field", "5", "--cluster_signed", "--cluster_min_weight", repr(floor_d), "--site_out", "s.tsv",
            "--prune_out", "p.txt")
    assert r.returncode == 0, r.stderr[-2000:]
    ids_d, _ = cluster_ref.clusters(table.decode(), labels, field=5, abs_value=False, min_weight=floor_d)
    assert open(tmp_path / "c3.tsv").read() == cluster_ref.cluster_file(ids_d, labels)
    assert os.path.getsize(tmp_path / "s.tsv") > 0 and os.path.getsize(tmp_path / "p.txt") > 0
    # without --pos no dist is finite: every node is a cluster of its own, and the sites are numbered from 1
    nopos = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--max_kb_dist", "0", "--max_snp_dist", "20"]
    r = subprocess.run([*nopos, "--cluster_out", "c4.tsv", "--cluster_table", "k4.tsv"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(tmp_path / "c4.tsv").read().splitlines()
    assert len(lines) == n_sites + 1 and lines[:4] == ["site\tcluster", "1\t1", "2\t2", "3\t3"]
    assert open(tmp_path / "k4.tsv").read() == cluster_ref.HEADER + "\n"
    # a matrix cut into slabs is refused before any pair is computed
    r = run("--cluster_out", "c5.tsv", env={**env, "NGSLD_TEST_SLAB_SITES": "100"})
    assert r.returncode == 255 and "--cluster_out needs the whole matrix resident on one device" in r.stderr, r.stderr[-1000:]
    assert not os.path.exists(tmp_path / "c5.tsv")
