"""LD across chromosomes on one MI355X: the phases of ngsld_cross_ld on all-pairs jobs -- BASELINE configs[1] at full size (5,000
sites x 100 individuals) with its sites dealt over 8 chromosomes, and 20,000 sites at configs[3]'s cohort size (1,000
individuals) over 8 chromosomes -- each at one bin per chromosome (B = 0) and at a B that gives about 1,000 bins, with r2 alone
and with all four statistics.  Per setting: the kernel with a wavefront's span of items M = 1 (one set of atomics per run:
grid.hip's global form, the yardstick), at the library's default M and at the other M of SPANS, three calls each, alternating;
the pair phase and the whole call of the default; and ngsld_grid's kernel over the same records in the same process (the
same-chromosome cells only: it drops the rows across chromosomes after reading them).

    python tools/cross_time.py [OUT_DIR]       (default profiles/cross; one JSON document, also printed)
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
SPAN_KNOB = "NGSLD_TEST_CROSS_SPAN_ITEMS"


def genome(n_sites, n_chr, seed):
    chrs, pos = synth.make_positions(n_sites, seed, max_gap=200, n_chr=n_chr)
    return chrs, pos


def one_call(eng, labels, bin_size, kw, span):
    os.environ.pop(SPAN_KNOB, None)
    if span is not None:
        os.environ[SPAN_KNOB] = str(span)
    try:
        t0 = time.perf_counter()
        cells, st = eng.cross_ld(labels, bin_size, **kw)
        st["wall_s"] = time.perf_counter() - t0
    finally:
        os.environ.pop(SPAN_KNOB, None)
    return cells, st


def summary(sts):
    best = min(sts, key=lambda s: s["cross_ms"])
    return {"span_items": best["span_items"], "chunks": best["chunks"], "cross_ms": best["cross_ms"],
            "cross_ms_all": [round(s["cross_ms"], 3) for s in sts], "pairs_ms": best["pairs_ms"], "total_ms": best["total_ms"],
            "pairs_ms_all": [round(s["pairs_ms"], 2) for s in sts], "total_ms_all": [round(s["total_ms"], 2) for s in sts],
            "cross_share_of_pairs": best["cross_ms"] / best["pairs_ms"], "call_over_pairs": best["total_ms"] / best["pairs_ms"]}


def timed_cross(raw, chrs, pos, runs, spans, reps=3):
    eng = capi.Engine(0)
    out = {}
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(extend_out=False)         # (all pairs: no window)
        t0 = time.perf_counter()
        eng.run_discard()                                 # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        out["pair_kernels_ms"] = eng.last_kernel_time()[0]
        for name, bin_size, kw in runs:
            one_call(eng, labels, bin_size, kw, None)     # (warm caches and allocator)
            res = {None: [], **{m: [] for m in spans}}
            first = {}
            for _ in range(reps):                         # alternating: every span sees the same box in the same minute
                for m in res:
                    cells, st = one_call(eng, labels, bin_size, kw, m)
                    res[m].append(st)
                    first.setdefault(m, cells)
            for m in first:                               # faster and different is not faster
                for k in first[None]:
                    a, b = first[None][k], first[m][k]
                    assert (a.tobytes() == b.tobytes()) if a.dtype.kind != "U" else (list(a) == list(b)), (m, k)
            s0 = res[None][0]
            entry = {"bin_size": bin_size, "bins": s0["bins"], "cells": s0["cells"], "pairs_counted": s0["pairs_counted"],
                     "pairs_cross": s0["pairs_cross"], "default": summary(res[None]),
                     "spans": {str(m): summary(res[m]) for m in spans}}
            entry["span1_over_default_cross_ms"] = entry["spans"]["1"]["cross_ms"] / entry["default"]["cross_ms"]
            # the grid's kernel over the same records (its own bins: one per chromosome is a bin_size beyond every position)
            gb = bin_size if bin_size else (1 << 31) - 1
            gst = [eng.grid(labels, gb, **kw)[1] for _ in range(reps)]
            entry["grid"] = {"lds": gst[0]["lds"], "band": gst[0]["band"], "grid_ms": min(s["grid_ms"] for s in gst),
                             "grid_ms_all": [round(s["grid_ms"], 3) for s in gst], "pairs_counted": gst[0]["pairs_counted"],
                             "total_ms": min(s["total_ms"] for s in gst)}
            out[name] = entry
            print(f"  {name}: default M {entry['default']['span_items']} {entry['default']['cross_ms']:.3f} ms, M=1 "
                  f"{entry['spans']['1']['cross_ms']:.3f} ms, grid {entry['grid']['grid_ms']:.3f} ms, pairs "
                  f"{entry['default']['pairs_ms']:.1f} ms, call {entry['default']['total_ms']:.1f} ms", flush=True)
    finally:
        eng.close()
    return out


def save(out_dir, res):
    """(after every input: a later one that fails does not take the earlier ones with it)"""
    with open(os.path.join(out_dir, "cross_time.json"), "w") as fh:
        fh.write(json.dumps(res, indent=1, default=float) + "\n")
    print(f"{list(res)[-1]}: done", flush=True)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "cross")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    for name, n_sites, n_ind, seed, spans in (("configs1_8chr_all_pairs", 5_000, 100, 1, (1, 2, 4, 8, 16, 32, 64, 256)),
                                             ("n20000_x1000_8chr_all_pairs", 20_000, 1_000, 3, (1, 4, 16, 64))):
        chrs, pos = genome(n_sites, 8, seed)
        per = -(-n_sites // 8)
        span_bp = int(sum(int(pos[min(n_sites, (c + 1) * per) - 1]) for c in range(8)))
        B = max(1, span_bp // 1000)                         # about 1,000 bins over the eight chromosomes
        runs = [(f"B{b}_{n}", b, kw) for b in (0, B) for n, kw in (("r2", {}), ("all4", dict(ld=ALL4)))]
        raw = synth.make_gl_numpy(n_sites, n_ind, seed, depth=10.0)
        print(f"{name}: {n_sites} sites x {n_ind}, B = {B}", flush=True)
        res[name] = timed_cross(raw, chrs, pos, runs, spans)
        res[name]["n_sites"], res[name]["n_ind"], res[name]["bin_size"] = n_sites, n_ind, B
        save(out_dir, res)
        del raw
    print(json.dumps(res, indent=1, default=float))


if __name__ == "__main__":
    main()
