"""LD partners on one MI355X: the phases of ngsld_partners on BASELINE configs[2] at full size (100,000 sites x 500
individuals, 100 kb window) and on its un-called twin (20 % monomorphic sites) -- r2 at k = 1, 10 and 64 and at floors 0.5, 0.2
and -inf, best of three calls each -- beside ngsld_site_ld's kernel and ngsld_linked_pairs' three kernels over the same records
in the same process.

    python tools/partners_time.py [OUT_DIR]       (default profiles/partners; one JSON document, also printed)
"""
from __future__ import annotations

import json
import math
import os
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from ngsld_amd import capi, shard, synth  # noqa: E402

KS = (1, 10, 64)
FLOORS = (0.5, 0.2, -math.inf)


def timed(raw, chrs, pos, max_kb, reps=3, others=True):
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
        eng.partners(1)                                 # (warm caches and allocator)
        for floor in FLOORS:
            for k in KS:
                sts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    res, st = eng.partners(k, min_weight=floor)
                    st["wall_s"] = time.perf_counter() - t0
                    sts.append(st)
                best = min(sts, key=lambda s: s["kernel_ms"])
                out[f"floor_{floor}_k{k}"] = {
                    "rows_counted": best["rows_counted"], "row_share": best["rows_counted"] / best["pairs"],
                    "sites_with_partners": best["sites_with_partners"], "entries": best["entries"], "chunks": best["chunks"],
                    "kernel_ms_all": [round(s["kernel_ms"], 3) for s in sts], "pairs_ms_all": [round(s["pairs_ms"], 2) for s in sts],
                    "total_ms_all": [round(s["total_ms"], 2) for s in sts],
                    "kernel_ms": best["kernel_ms"], "pairs_ms": best["pairs_ms"], "total_ms": best["total_ms"],
                    "kernel_share_of_pairs": best["kernel_ms"] / best["pairs_ms"], "call_over_pairs": best["total_ms"] / best["pairs_ms"],
                    "first_site": [int(res["rows"][0]), res["partner"][0, :3].tolist(), res["value_micro"][0, :3].tolist()]}
        if others:                                      # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2):
                _, sst = eng.site_ld()
            out["site_ld_r2"] = {k: sst[k] for k in ("site_ms", "pairs_ms", "total_ms", "lds")}
            for floor in (0.5, 0.2):
                for _ in range(2):
                    _, lst = eng.linked_pairs(None, min_weight=floor, records=True)
                out[f"linked_r2_floor_{floor}"] = {k: lst[k] for k in ("rows", "count_ms", "scan_ms", "write_ms", "kernel_ms", "pairs_ms",
                                                                        "total_ms")}
            for floor in (0.5, 0.2):
                for k in KS:
                    e = out[f"floor_{floor}_k{k}"]
                    e["kernel_ms_over_site_ms"] = e["kernel_ms"] / sst["site_ms"]
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "partners")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed(raw, chrs, pos, 100)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed(twin, chrs, pos, 100, others=False)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "partners_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
