"""The LD grid on one MI355X: the phases of ngsld_grid on BASELINE configs[2] at full size (100,000 sites x 500 individuals, 100 kb
window) and on its un-called twin (20 % monomorphic sites) at bin sizes 10,000 and 1,000, with r2 alone and with all four
statistics, each with the tile's cells in LDS wherever 64 KiB hold them and forced to global atomics (alternating, three calls
each; "shipped" says which of the two the library takes by itself), beside
ngsld_site_ld's and ngsld_decay's kernels over the same records in the same process; and on all pairs of configs[1] (5,000 sites x
100 individuals, no window: the band is the whole chromosome) at a bin size of 1,000, whose accumulators (some 250,000 cells)
stay far below the 2 GiB limit -- with one, two and four statistics: 48 KB of window a tile, and two that no LDS holds.

    python tools/grid_time.py [OUT_DIR]       (default profiles/grid; one JSON document, also printed)
"""
from __future__ import annotations

import json
import os
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from ngsld_amd import capi, shard, synth  # noqa: E402

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
LDS_KNOB = "NGSLD_TEST_GRID_LDS_BYTES"


def one_call(eng, labels, bin_size, kw, lds_bytes):
    os.environ.pop(LDS_KNOB, None)
    if lds_bytes is not None:
        os.environ[LDS_KNOB] = str(lds_bytes)
    try:
        t0 = time.perf_counter()
        cells, st = eng.grid(labels, bin_size, **kw)
        st["wall_s"] = time.perf_counter() - t0
    finally:
        os.environ.pop(LDS_KNOB, None)
    return cells, st


def timed_grid(raw, chrs, pos, max_kb, runs, reps=3, others=True):
    eng = capi.Engine(0)
    out = {}
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(max_kb_dist=max_kb, extend_out=False)
        t0 = time.perf_counter()
        eng.run_discard()                               # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        out["pair_kernels_ms"] = eng.last_kernel_time()[0]
        for name, bin_size, kw in runs:
            one_call(eng, labels, bin_size, kw, None)   # (warm caches and allocator)
            _, shipped = one_call(eng, labels, bin_size, kw, None)
            res = {"lds": [], "global": []}
            first = {}
            for _ in range(reps):                       # alternating: the two paths see the same box in the same minute
                for path, knob in (("lds", 65536), ("global", 0)):
                    cells, st = one_call(eng, labels, bin_size, kw, knob)
                    res[path].append(st)
                    if path not in first:
                        first[path] = cells
            for k in first["lds"]:                      # faster and different is not faster
                assert first["lds"][k].tobytes() == first["global"][k].tobytes(), k
            entry = {"bin_size": bin_size, "shipped": "lds" if shipped["lds"] else "global"}
            for path, sts in res.items():
                best = min(sts, key=lambda s: s["grid_ms"])
                entry[path] = {"lds": best["lds"], "chunks": best["chunks"], "pairs_counted": best["pairs_counted"],
                               "cells": best["cells"], "bins": best["bins"], "band": best["band"],
                               "grid_ms_all": [round(s["grid_ms"], 3) for s in sts],
                               "pairs_ms_all": [round(s["pairs_ms"], 2) for s in sts],
                               "total_ms_all": [round(s["total_ms"], 2) for s in sts],
                               "grid_ms": best["grid_ms"], "pairs_ms": best["pairs_ms"], "total_ms": best["total_ms"],
                               "grid_share_of_pairs": best["grid_ms"] / best["pairs_ms"],
                               "call_over_pairs": best["total_ms"] / best["pairs_ms"]}
            entry["global_over_lds_grid_ms"] = entry["global"]["grid_ms"] / entry["lds"]["grid_ms"]
            c = first["lds"]
            f = [x for x in ALL4 if f"sum_{x}" in c][-1]
            entry["first_cells"] = [[str(c["chr"][k]), int(c["bin1"][k]), int(c["bin2"][k]), int(c["n"][k]), int(c[f"sum_{f}"][k]),
                                     float(c[f"mean_{f}"][k]), int(c[f"linked_{f}"][k])] for k in range(min(3, len(c["n"])))]
            out[name] = entry
        if others:                                      # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2):
                _, sst = eng.site_ld()
            out["site_ld_r2"] = {k: sst[k] for k in ("site_ms", "pairs_ms", "total_ms", "lds")}
            for _ in range(2):
                _, dst = eng.decay()
            out["decay_r2"] = {k: dst[k] for k in ("bin_ms", "pairs_ms", "total_ms", "lds")}
            for name, _, _ in runs:
                out[name]["grid_ms_over_site_ms"] = out[name][out[name]["shipped"]]["grid_ms"] / sst["site_ms"]
                out[name]["grid_ms_over_decay_bin_ms"] = out[name][out[name]["shipped"]]["grid_ms"] / dst["bin_ms"]
    finally:
        eng.close()
    return out


def save(out_dir, res):
    """(after every input: a later one that fails does not take the earlier ones with it)"""
    with open(os.path.join(out_dir, "grid_time.json"), "w") as fh:
        fh.write(json.dumps(res, indent=1, default=float) + "\n")
    print(f"{list(res)[-1]}: done", flush=True)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "grid")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    runs = [(f"B{b}_{n}", b, kw) for b in (10_000, 1_000) for n, kw in (("r2", {}), ("all4", dict(ld=ALL4)))]
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_grid(raw, chrs, pos, 100, runs)
    save(out_dir, res)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_grid(twin, chrs, pos, 100, runs, others=False)
    save(out_dir, res)
    del twin
    c1, p1 = synth.make_positions(5_000, 1, max_gap=200)
    raw1 = synth.make_gl_numpy(5_000, 100, 1, depth=10.0)
    runs1 = [("B1000_r2", 1_000, {}), ("B1000_Dp_r2", 1_000, dict(ld=("Dp", "r2"))), ("B1000_all4", 1_000, dict(ld=ALL4))]
    res["configs1_all_pairs"] = timed_grid(raw1, c1, p1, 0, runs1, others=False)
    save(out_dir, res)
    print(json.dumps(res, indent=1, default=float))


if __name__ == "__main__":
    main()
