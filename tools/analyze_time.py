"""Six analyses singly and in one ngsld_analyze on one MI355X: BASELINE configs[2] at full size (100,000 sites x 500
individuals, 100 kb window) and its un-called twin (20 % monomorphic sites).  LD pruning (min_weight 0.5), decay, site LD,
clusters, the grid (10 kb windows) and the scan (half window 5 kb), each with its documented defaults otherwise: the six single
calls one after the other, then Engine.analyze with the same six, in the same process on the same context (three rounds each,
the best kept).  ANALYZE.md holds the table.

    python tools/analyze_time.py [OUT_DIR]       (default profiles/analyze; one JSON document, also printed)
"""
from __future__ import annotations

import json
import os
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from ngsld_amd import capi, shard, synth  # noqa: E402

NAMES = ("prune", "decay", "site_ld", "clusters", "grid", "scan")
KERNEL_MS = dict(prune="edges_ms", decay="bin_ms", site_ld="site_ms", clusters="union_ms", grid="grid_ms", scan="scan_ms")


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(raw, chrs, pos, reps=3):
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    kw = dict(prune=dict(labels=labels, min_weight=0.5), decay={}, site_ld={}, clusters={}, grid=dict(labels=labels, bin_size=10_000),
              scan=dict(half_window=5_000))
    eng = capi.Engine(0)
    out = {}
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(max_kb_dist=100, extend_out=False)
        t0 = time.perf_counter()
        eng.run_discard()                               # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        eng.analyze(**kw)                               # (warm caches and allocator)
        singles, bundles = [], []
        for _ in range(reps):
            one = {}
            t_all = time.perf_counter()
            for name in NAMES:
                t0 = time.perf_counter()
                st = getattr(eng, name)(**kw[name])[-1]
                one[name] = {"wall_ms": (time.perf_counter() - t0) * 1e3, "total_ms": st["total_ms"], "pairs_ms": st["pairs_ms"],
                             "kernel_ms": st[KERNEL_MS[name]]}
            one["wall_ms"] = (time.perf_counter() - t_all) * 1e3
            singles.append(one)
            t0 = time.perf_counter()
            res, ast = eng.analyze(**kw)
            ast["wall_ms"] = (time.perf_counter() - t0) * 1e3
            ast["per_pass"] = {name: {"total_ms": res[name][-1]["total_ms"], "kernel_ms": res[name][-1][KERNEL_MS[name]]} for name in NAMES}
            bundles.append(ast)
        s, b = min(singles, key=lambda x: x["wall_ms"]), min(bundles, key=lambda x: x["wall_ms"])
        out["singles"], out["bundle"] = s, b
        out["singles_wall_ms_all"] = [round(x["wall_ms"], 1) for x in singles]
        out["bundle_wall_ms_all"] = [round(x["wall_ms"], 1) for x in bundles]
        mean_single = s["wall_ms"] / len(NAMES)
        out["six_singles_over_bundle"] = s["wall_ms"] / b["wall_ms"]
        out["bundle_over_mean_single"] = b["wall_ms"] / mean_single
        say(f"  six singles {s['wall_ms']:.1f} ms, bundle {b['wall_ms']:.1f} ms (pairs {b['pairs_ms']:.1f}, kernels {b['kernels_ms']:.1f}; "
            f"pairs_run {b['pairs_run']} of {b['pairs']}): {out['six_singles_over_bundle']:.2f}x, "
            f"{out['bundle_over_mean_single']:.2f} of a mean single call")
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "analyze")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    say("configs[2]")
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed(raw, chrs, pos)
    del raw
    say("un-called twin")
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed(twin, chrs, pos)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "analyze_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
