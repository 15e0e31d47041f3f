"""The LD scan on one MI355X: the phases of ngsld_scan on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window) and on its un-called twin (20 % monomorphic sites), at half windows of 5 kb and 50 kb, r2 alone and all four
statistics (three calls each, the best kept), beside ngsld_site_ld's kernel -- with its LDS tiles and forced to global atomics --
and ngsld_decay's bin kernel over the same records in the same process; and on all pairs of configs[1] (5,000 sites x 100
individuals, no window).

    python tools/scan_time.py [OUT_DIR]       (default profiles/scan; one JSON document, also printed)
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
SITE_LDS_KNOB = "NGSLD_TEST_SITE_LDS_BYTES"


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed_scans(raw, chrs, pos, max_kb, halves, reps=3, others=True):
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
        for half in halves:
            for name, kw in (("r2", {}), ("all4", dict(ld=ALL4))):
                eng.scan(half, **kw)                    # (warm caches and allocator)
                sts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    win, st = eng.scan(half, **kw)
                    st["wall_s"] = time.perf_counter() - t0
                    sts.append(st)
                best = min(sts, key=lambda s: s["scan_ms"])
                f = "r2"
                entry = {"half_window": half, "chunks": best["chunks"], "pairs_counted": best["pairs_counted"],
                         "largest_window": best["largest_window"],
                         "scan_ms_all": [round(s["scan_ms"], 3) for s in sts],
                         "pairs_ms_all": [round(s["pairs_ms"], 2) for s in sts],
                         "total_ms_all": [round(s["total_ms"], 2) for s in sts],
                         "scan_ms": best["scan_ms"], "pairs_ms": best["pairs_ms"], "total_ms": best["total_ms"],
                         "scan_share_of_pairs": best["scan_ms"] / best["pairs_ms"],
                         "call_over_pairs": best["total_ms"] / best["pairs_ms"],
                         "host_ms": best["total_ms"] - best["pairs_ms"] - best["scan_ms"],
                         "middle_sites": [[int(win["n_ll"][k]), int(win["n_rr"][k]), int(win["n_lr"][k]), float(win[f"zns_{f}"][k]),
                                           float(win[f"omega_{f}"][k])] for k in (len(chrs) // 2, len(chrs) // 2 + 1)]}
                out[f"H{half}_{name}"] = entry
                say(f"  H {half} {name}: scan {best['scan_ms']:.2f} ms, pairs {best['pairs_ms']:.1f} ms, call {best['total_ms']:.1f} ms")
        if others:                                      # the kernels that read the same 32 B a pair, same process, same box
            for label, knob in (("site_ld_r2", None), ("site_ld_r2_global", "0")):
                os.environ.pop(SITE_LDS_KNOB, None)
                if knob is not None:
                    os.environ[SITE_LDS_KNOB] = knob
                try:
                    for _ in range(2):
                        _, sst = eng.site_ld()
                finally:
                    os.environ.pop(SITE_LDS_KNOB, None)
                out[label] = {k: sst[k] for k in ("site_ms", "pairs_ms", "total_ms", "lds")}
            for _ in range(2):
                _, dst = eng.decay()
            out["decay_r2"] = {k: dst[k] for k in ("bin_ms", "pairs_ms", "total_ms", "lds")}
            say(f"  site LD {out['site_ld_r2']['site_ms']:.2f} ms (global {out['site_ld_r2_global']['site_ms']:.2f} ms), "
                f"decay {dst['bin_ms']:.2f} ms")
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "scan")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    say("configs[2]")
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_scans(raw, chrs, pos, 100, (5_000, 50_000))
    del raw
    say("un-called twin")
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_scans(twin, chrs, pos, 100, (5_000, 50_000), others=False)
    del twin
    say("configs[1], all pairs")
    c1, p1 = synth.make_positions(5_000, 1, max_gap=200)
    raw1 = synth.make_gl_numpy(5_000, 100, 1, depth=10.0)
    res["configs1_all_pairs"] = timed_scans(raw1, c1, p1, 0, (50_000,), others=False)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "scan_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
