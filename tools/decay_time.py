"""LD decay on one MI355X: the phases of ngsld_decay on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window; r2 alone and all four statistics), on its un-called twin (20 % monomorphic sites), and on all pairs of
configs[1] (5,000 sites x 100 individuals, no window: the many-bins path at bin size 2 and the LDS path at 250), each beside
the pair phase alone; and the binary's wall time with --decay_out against --out.

    python tools/decay_time.py [OUT_DIR]       (default profiles/decay; one JSON document, also printed)
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

ALL4 = ("r2_ExpG", "D", "Dp", "r2")


def timed_decays(raw, chrs, pos, max_kb, runs):
    eng = capi.Engine(0)
    out = {}
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(max_kb_dist=max_kb, extend_out=False)
        t0 = time.perf_counter()
        eng.run_discard()                               # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        out["pair_kernels_ms"] = eng.last_kernel_time()[0]
        for name, kw in runs:
            best = None
            for _ in range(2):                          # (the second call is the one reported: warm caches and allocator)
                t0 = time.perf_counter()
                bins, st = eng.decay(**kw)
                st["wall_s"] = time.perf_counter() - t0
                best = st
            best["bin_share_of_pairs"] = best["bin_ms"] / best["pairs_ms"]
            best["call_over_pairs"] = best["total_ms"] / best["pairs_ms"]
            best["first_bins"] = [[float(bins["dist"][k]), int(bins["n"][k])] + [float(bins[f][k]) for f in ALL4 if f in bins]
                                  for k in range(min(3, len(bins["dist"])))]
            out[name] = best
    finally:
        eng.close()
    return out


def binary_wall(raw, chrs, pos, d, n_ind, max_kb):
    g, p = os.path.join(d, "g.bin"), os.path.join(d, "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(len(chrs)), "--pos", p, "--max_kb_dist",
            str(max_kb)]
    res = {}
    for name, extra in (("out_tsv", ["--out", "/dev/null"]),
                        ("decay_out", ["--decay_out", os.path.join(d, "b.tsv"), "--decay_fit", os.path.join(d, "f.tsv")])):
        t0 = time.perf_counter()
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        res[name + "_s"] = time.perf_counter() - t0
        if r.returncode != 0:
            res[name + "_error"] = r.stderr[-1000:]
        elif name == "decay_out":
            res["decay_stderr"] = [ln for ln in r.stderr.splitlines() if "LD decay" in ln]
            res["decay_fit"] = open(os.path.join(d, "f.tsv")).read().splitlines()
    return res


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "decay")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_decays(raw, chrs, pos, 100, [("r2", {}), ("all4", dict(ld=ALL4))])
    with tempfile.TemporaryDirectory() as d:
        res["configs2_binary"] = binary_wall(raw, chrs, pos, d, 500, 100)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_decays(twin, chrs, pos, 100, [("r2", {}), ("all4", dict(ld=ALL4))])
    del twin
    c1, p1 = synth.make_positions(5_000, 1, max_gap=200)
    raw1 = synth.make_gl_numpy(5_000, 100, 1, depth=10.0)
    res["configs1_all_pairs"] = timed_decays(raw1, c1, p1, 0, [("bin2_global", dict(bin_size=2)),
                                                                ("bin250_lds", dict(bin_size=250)),
                                                                ("bin2_all4_global", dict(bin_size=2, ld=ALL4))])
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "decay_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
