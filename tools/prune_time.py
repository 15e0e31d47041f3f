"""LD pruning on one MI355X: the phases of ngsld_prune on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window) at min_weight 0.2 and 0.5 and on its un-called twin (20 % monomorphic sites), the binary's wall time with
--prune_out against --out, and the Python restatement of prune_graph.pl (tests/prune_ref.py) on a 10,000-site slice for scale.

    python tools/prune_time.py [OUT_DIR]       (default profiles/prune; one JSON document, also printed)
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from ngsld_amd import capi, shard, synth  # noqa: E402

N_SITES, N_IND, MAX_KB, MAX_GAP, DEPTH = 100_000, 500, 100, 200, 10.0


def engine_for(raw, chrs, pos):
    eng = capi.Engine(0)
    eng.set_geno_raw(raw)
    eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
    n = eng.plan(max_kb_dist=MAX_KB, extend_out=False)
    return eng, n


def timed_prunes(raw, chrs, pos, weights):
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    eng, n = engine_for(raw, chrs, pos)
    out = {"pairs": n}
    try:
        t0 = time.perf_counter()
        eng.run_discard()                               # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        ms, _, _ = eng.last_kernel_time()
        out["pair_kernels_ms"] = ms
        for mw in weights:
            t0 = time.perf_counter()
            _, st = eng.prune(labels, min_weight=mw)
            st["wall_s"] = time.perf_counter() - t0
            out[f"min_weight_{mw}"] = st
    finally:
        eng.close()
    return out


def binary_wall(raw, chrs, pos, d):
    g, p = os.path.join(d, "g.bin"), os.path.join(d, "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(N_IND), "--n_sites", str(N_SITES), "--pos", p, "--max_kb_dist", str(MAX_KB)]
    res = {}
    for name, extra in (("out_tsv", ["--out", "/dev/null"]), ("prune_out", ["--prune_out", os.path.join(d, "kept"),
                                                                            "--prune_min_weight", "0.2"])):
        t0 = time.perf_counter()
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        res[name + "_s"] = time.perf_counter() - t0
        if r.returncode != 0:
            res[name + "_error"] = r.stderr[-1000:]
        elif name == "prune_out":
            res["prune_stderr"] = [ln for ln in r.stderr.splitlines() if "Pruning" in ln]
    return res


def ref_slice(raw, chrs, pos, n=10_000):
    import prune_ref
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs[:n], pos[:n])]
    eng, pairs = engine_for(raw[:n], chrs[:n], pos[:n])
    try:
        eng.set_text_output(labels)
        text, _ = eng.run_text()
        t0 = time.perf_counter()
        _, st = eng.prune(labels, min_weight=0.2)
        dev_s = time.perf_counter() - t0
    finally:
        eng.close()
    t0 = time.perf_counter()
    kept, excl = prune_ref.prune_tsv(text.decode(), min_weight=0.2)
    ref_s = time.perf_counter() - t0
    return {"sites": n, "pairs": pairs, "tsv_bytes": len(text), "prune_ref_s": ref_s, "ngsld_prune_s": dev_s,
            "same_counts": [len(kept), len(excl)] == [st["kept"], st["excluded"]]}


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "prune")
    os.makedirs(out_dir, exist_ok=True)
    chrs, pos = synth.make_positions(N_SITES, 2, max_gap=MAX_GAP)
    res = {"config": dict(sites=N_SITES, ind=N_IND, max_kb=MAX_KB, max_gap=MAX_GAP, depth=DEPTH)}
    raw = synth.make_gl_numpy(N_SITES, N_IND, 2, depth=DEPTH)
    res["configs2"] = timed_prunes(raw, chrs, pos, [0.2, 0.5])
    with tempfile.TemporaryDirectory() as d:
        res["binary"] = binary_wall(raw, chrs, pos, d)
    res["prune_ref_slice"] = ref_slice(raw, chrs, pos)
    del raw
    twin = synth.make_gl_numpy(N_SITES, N_IND, 2, depth=DEPTH, mono_frac=0.2)
    res["uncalled_twin"] = timed_prunes(twin, chrs, pos, [0.2])
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "prune_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
