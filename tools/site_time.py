"""Per-site LD summaries on one MI355X: the phases of ngsld_site_ld on BASELINE configs[2] at full size (100,000 sites x 500
individuals, 100 kb window; r2 alone and all four statistics) and on its un-called twin (20 % monomorphic sites), each with the
tile accumulators in LDS and forced to global atomics (alternating, three calls each), beside ngsld_decay's bin kernel and
ngsld_prune's edge extraction over the same records in the same process; and on all pairs of configs[1] (5,000 sites x 100
individuals, no window: the span does not fit, the global path).

    python tools/site_time.py [OUT_DIR]       (default profiles/sites; one JSON document, also printed)
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
LDS_KNOB = "NGSLD_TEST_SITE_LDS_BYTES"


def one_call(eng, kw, lds_bytes):
    os.environ.pop(LDS_KNOB, None)
    if lds_bytes is not None:
        os.environ[LDS_KNOB] = str(lds_bytes)
    try:
        t0 = time.perf_counter()
        sites, st = eng.site_ld(**kw)
        st["wall_s"] = time.perf_counter() - t0
    finally:
        os.environ.pop(LDS_KNOB, None)
    return sites, st


def timed_sites(raw, chrs, pos, max_kb, runs, reps=3, others=True):
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
            one_call(eng, kw, None)                     # (warm caches and allocator)
            res = {"default": [], "global": []}
            first = {}
            for _ in range(reps):                       # alternating: the two paths see the same box in the same minute
                for path, knob in (("default", None), ("global", 0)):
                    sites, st = one_call(eng, kw, knob)
                    res[path].append(st)
                    if path not in first:
                        first[path] = sites
            for k in first["default"]:                  # faster and different is not faster
                assert first["default"][k].tobytes() == first["global"][k].tobytes(), k
            entry = {}
            for path, sts in res.items():
                best = min(sts, key=lambda s: s["site_ms"])
                entry[path] = {"lds": best["lds"], "chunks": best["chunks"], "pairs_counted": best["pairs_counted"],
                               "sites_with_pairs": best["sites_with_pairs"],
                               "site_ms_all": [round(s["site_ms"], 3) for s in sts],
                               "pairs_ms_all": [round(s["pairs_ms"], 2) for s in sts],
                               "total_ms_all": [round(s["total_ms"], 2) for s in sts],
                               "site_ms": best["site_ms"], "pairs_ms": best["pairs_ms"], "total_ms": best["total_ms"],
                               "site_share_of_pairs": best["site_ms"] / best["pairs_ms"],
                               "call_over_pairs": best["total_ms"] / best["pairs_ms"]}
            entry["global_over_default_site_ms"] = entry["global"]["site_ms"] / entry["default"]["site_ms"]
            s = first["default"]
            f = [x for x in ALL4 if f"sum_{x}" in s][-1]
            entry["first_sites"] = [[int(s["n"][k]), int(s[f"sum_{f}"][k]), float(s[f"mean_{f}"][k]), int(s[f"linked_{f}"][k])]
                                    for k in range(min(3, len(s["n"])))]
            out[name] = entry
        if others:                                      # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2):
                _, dst = eng.decay()
            out["decay_r2"] = {k: dst[k] for k in ("bin_ms", "pairs_ms", "total_ms", "lds")}
            labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
            for _ in range(2):
                _, pst = eng.prune(labels, min_weight=0.5)
            out["prune_r2"] = {k: pst[k] for k in ("edges_ms", "pairs_ms", "total_ms", "edges")}
            for name, _ in runs:
                out[name]["site_ms_over_decay_bin_ms"] = out[name]["default"]["site_ms"] / dst["bin_ms"]
                out[name]["site_ms_over_prune_edges_ms"] = out[name]["default"]["site_ms"] / pst["edges_ms"]
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "sites")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    runs = [("r2", {}), ("all4", dict(ld=ALL4))]
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_sites(raw, chrs, pos, 100, runs)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_sites(twin, chrs, pos, 100, runs, others=False)
    del twin
    c1, p1 = synth.make_positions(5_000, 1, max_gap=200)
    raw1 = synth.make_gl_numpy(5_000, 100, 1, depth=10.0)
    res["configs1_all_pairs"] = timed_sites(raw1, c1, p1, 0, runs, others=False)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "site_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
