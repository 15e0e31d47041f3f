"""LD pruning on the device (ngsld_prune, Engine.prune, the binary's --prune_* flags) against tests/prune_ref.py -- the
restatement of prune_graph.pl -- applied to the same engine's own TSV (run_text).  Kept and excluded sets must be equal."""
import os
import subprocess

import numpy as np
import pytest

import prune_ref
from ngsld_amd import capi, shard, synth

pytestmark = pytest.mark.gpu


def _labels(chrs, pos):
    return [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]


def _case(raw, chrs, pos, plan_kw, prune_kw, geno_kw=None, labels=None):
    """Engine.prune against prune_ref over the engine's own TSV; returns the stats."""
    labels = labels or _labels(chrs, pos)
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw, **(geno_kw or {}))
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        eng.plan(**plan_kw)
        eng.set_text_output(labels)
        text, fallbacks = eng.run_text()
        assert fallbacks == 0
        state, stats = eng.prune(labels, **prune_kw)
    finally:
        eng.close()
    ref_kw = {k: v for k, v in prune_kw.items() if k != "keep_heavy"}
    if "subset" in ref_kw:
        ref_kw["subset"] = set(ref_kw["subset"])
    kept, excl = prune_ref.prune_tsv(text.decode(), keep_heavy=prune_kw.get("keep_heavy", False), **ref_kw)
    got_kept = {labels[s] for s in np.nonzero(state == 1)[0]}
    got_excl = {labels[s] for s in np.nonzero(state == 2)[0]}
    assert got_kept == kept and got_excl == excl, (len(got_kept ^ kept), len(got_excl ^ excl))
    assert stats["nodes"] == stats["kept"] + stats["excluded"] == len(kept) + len(excl)
    return stats


WIN = dict(max_kb_dist=20, extend_out=False)
CASES = {
    # name: (n_sites, n_ind, synth kw, n_chr, plan kw, prune kw, geno kw)
    "n8_window": (500, 8, {}, 1, WIN, {}, None),
    "n64_window_mw005": (500, 64, {}, 1, WIN, dict(min_weight=0.05), None),
    "n500_window_mw03": (400, 500, {}, 1, WIN, dict(min_weight=0.3), None),
    "allpairs_two_chr": (300, 64, {}, 2, dict(extend_out=False), {}, None),
    "allpairs_kb_limit": (300, 8, {}, 1, dict(extend_out=True), dict(max_kb_dist=3.5), None),
    "min_maf_rnd_sample": (500, 64, {}, 2, dict(max_kb_dist=30, min_maf=0.1, rnd_sample=0.6, seed=7), {}, None),
    "field4": (400, 64, {}, 1, WIN, dict(field=4, min_weight=0.05), None),
    "field5_e": (400, 64, {}, 1, WIN, dict(field=5, weight_type="e"), None),
    "field5_e_negative": (400, 64, {}, 1, WIN, dict(field=5, weight_type="e", min_weight=-1.0), None),
    "field6_a": (400, 8, {}, 1, WIN, dict(field=6), None),
    "field6_e_negative": (300, 8, {}, 1, WIN, dict(field=6, weight_type="e", min_weight=-2.0), None),
    "type_n": (400, 64, {}, 1, WIN, dict(weight_type="n", min_weight=0.3), None),
    "keep_heavy": (400, 64, {}, 1, WIN, dict(keep_heavy=True, min_weight=0.05), None),
    "keep_heavy_n": (400, 8, {}, 1, WIN, dict(keep_heavy=True, weight_type="n", min_weight=0.3), None),
    "precision_2": (400, 64, {}, 1, WIN, dict(precision=2), None),
    "uncalled_mono": (500, 64, dict(mono_frac=0.2), 1, WIN, {}, None),
    "uncalled_mono_field6": (400, 64, dict(mono_frac=0.2), 1, WIN, dict(field=6, min_weight=0.3), None),
    "call_geno": (500, 64, {}, 1, WIN, dict(min_weight=0.05), dict(call_geno=(0.1, 0.9))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_prune_equals_script_on_own_tsv(name):
    n_sites, n_ind, skw, n_chr, plan_kw, prune_kw, geno_kw = CASES[name]
    raw = synth.make_gl_numpy(n_sites, n_ind, 300 + n_sites + n_ind, depth=4.0, **skw)
    chrs, pos = synth.make_positions(n_sites, 31, max_gap=300, n_chr=n_chr)
    _case(raw, chrs, pos, plan_kw, prune_kw, geno_kw)


def test_subset():
    raw = synth.make_gl_numpy(400, 64, 17, depth=4.0)
    chrs, pos = synth.make_positions(400, 17, max_gap=300)
    labels = _labels(chrs, pos)
    subset = [lab for k, lab in enumerate(labels) if k % 3 != 1] + ["not_a_site"]
    _case(raw, chrs, pos, WIN, dict(subset=subset, min_weight=0.05))


def test_mixed_case_labels_and_duplicated_sites():
    """Two chromosomes whose names differ in case only, the same genotypes at the same positions on both: every weight is tied
    between the copies, and lc(label) ties too -- the raw bytes decide (PRUNE.md)."""
    half = synth.make_gl_numpy(200, 64, 23, depth=4.0)
    half[1::7] = half[0::7][: len(half[1::7])]          # duplicated neighbouring sites as well
    raw = np.concatenate([half, half])
    _, p = synth.make_positions(200, 23, max_gap=300)
    chrs = ["Chr1"] * 200 + ["chr1"] * 200
    pos = np.concatenate([p, p])
    stats = _case(raw, chrs, pos, WIN, {})
    assert stats["excluded"] > 0


def test_chain_with_host_finish_forced(monkeypatch):
    """max_snp_dist 1 makes a chain (a round per node in the worst case); the host finishes after two device rounds."""
    raw = synth.make_gl_numpy(600, 64, 41, depth=4.0)
    chrs, pos = synth.make_positions(600, 41, max_gap=300)
    for after in ("2", "0"):
        monkeypatch.setenv("NGSLD_TEST_PRUNE_HOST_AFTER", after)
        stats = _case(raw, chrs, pos, dict(max_snp_dist=1, extend_out=False), {})
        assert stats["rounds"] <= int(after) and (after != "0" or stats["host_nodes"] > 0)


def test_device_rounds_do_the_bulk():
    raw = synth.make_gl_numpy(600, 64, 43, depth=4.0)
    chrs, pos = synth.make_positions(600, 43, max_gap=300)
    stats = _case(raw, chrs, pos, WIN, {})
    assert stats["rounds"] >= 1 and stats["edges"] > 0 and stats["host_nodes"] < stats["nodes"]


def test_duplicate_label_is_refused():
    raw = synth.make_gl_numpy(100, 8, 5, depth=4.0)
    chrs, pos = synth.make_positions(100, 5, max_gap=300)
    labels = _labels(chrs, pos)
    labels[50] = labels[20]
    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        eng.plan(**WIN)
        with pytest.raises(capi.NgsldError) as e:
            eng.prune(labels)
        assert e.value.code == capi.ERR_INVALID and labels[20] in e.value.msg
    finally:
        eng.close()


def test_cli_prune_equals_script_and_leaves_tsv_alone(tmp_path):
    n_sites, n_ind = 500, 64
    raw = synth.make_gl_numpy(n_sites, n_ind, 77, depth=4.0, mono_frac=0.1)
    chrs, pos = synth.make_positions(n_sites, 77, max_gap=300, n_chr=2)
    g, p = str(tmp_path / "g.bin"), str(tmp_path / "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "20"]
    run = lambda *a: subprocess.run([*base, *a], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)  # noqa: E731
    r = run("--out", "t.tsv")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("--prune_out", "k", "--prune_excl", "x", "--prune_min_weight", "0.05")
    assert r.returncode == 0, r.stderr[-2000:]
    tsv = open(tmp_path / "t.tsv").read()
    kept, excl = prune_ref.prune_tsv(tsv, min_weight=0.05)
    got_k = open(tmp_path / "k").read().split("\n")[:-1]
    got_x = open(tmp_path / "x").read().split("\n")[:-1]
    assert set(got_k) == kept and set(got_x) == excl and len(got_k) == len(kept) and len(got_x) == len(excl)
    r = run("--out", "t2.tsv", "--prune_out", "k2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "t2.tsv", "rb").read() == open(tmp_path / "t.tsv", "rb").read()
    assert set(open(tmp_path / "k2").read().split("\n")[:-1]) == prune_ref.prune_tsv(tsv)[0]
    assert not os.path.exists(tmp_path / "t3.tsv")
