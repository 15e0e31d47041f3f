"""The LD decay map on one MI355X: the phases of ngsld_decay_map on BASELINE configs[2] at full size (100,000 sites x 500
individuals, 100 kb window: one chromosome of some 10 Mb) and on its un-called twin (20 % monomorphic sites) -- r2 alone and all
four statistics; a group per chromosome, per window of 1 Mb and per window of 100 kb; both kernel forms (LDS for the home group,
every add to global memory) -- beside ngsld_decay with the same parameters in the same process, the host's share of the call (the
copy back, the means) and the time of the per-group fits; and the binary's wall time with --dmap_out and with --dmap_fit too.

    python tools/dmap_time.py [OUT_DIR]       (default profiles/dmap; one JSON document, also printed)
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
WINDOWS = (("chromosome", 0), ("1Mb", 1_000_000), ("100kb", 100_000))


def second_call(fn):
    """(result, wall seconds) of the second of two calls: warm caches and allocator."""
    fn()
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def timed_maps(raw, chrs, pos, max_kb):
    labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
    eng = capi.Engine(0)
    out = {}
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(max_kb_dist=max_kb, extend_out=False)
        t0 = time.perf_counter()
        eng.run_discard()                               # the pair kernels + hand-off once (warm-up, and the pair phase alone)
        out["run_discard_s"] = time.perf_counter() - t0
        for ld_name, ld in (("r2", ("r2",)), ("all4", ALL4)):
            (_, st), wall = second_call(lambda: eng.decay(ld=ld))
            st.update(wall_s=wall, bin_share_of_pairs=st["bin_ms"] / st["pairs_ms"], call_over_pairs=st["total_ms"] / st["pairs_ms"])
            out[f"decay_{ld_name}"] = st
            for w_name, window in WINDOWS:
                for form, lds_bytes in (("lds", None), ("global", "0")):
                    os.environ.pop("NGSLD_TEST_DMAP_LDS_BYTES", None)
                    if lds_bytes is not None:
                        os.environ["NGSLD_TEST_DMAP_LDS_BYTES"] = lds_bytes
                    (groups, st), wall = second_call(lambda: eng.decay_map(labels, window=window, ld=ld))
                    os.environ.pop("NGSLD_TEST_DMAP_LDS_BYTES", None)
                    st.update(wall_s=wall, kernel_share_of_pairs=st["kernel_ms"] / st["pairs_ms"],
                              call_over_pairs=st["total_ms"] / st["pairs_ms"],
                              host_ms=st["total_ms"] - st["pairs_ms"] - st["kernel_ms"])  # the site arrays, the copy back, the means
                    if form == "lds":
                        t0 = time.perf_counter()
                        fits = capi.decay_map_fit(groups, "r2")
                        st["fit_r2_s"] = time.perf_counter() - t0
                        st["groups_fitted"] = sum(f is not None for f in fits)
                    out[f"map_{ld_name}_{w_name}_{form}"] = st
    finally:
        eng.close()
    return out


def binary_wall(raw, chrs, pos, d, n_ind, max_kb):
    g, p = os.path.join(d, "g.bin"), os.path.join(d, "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(len(chrs)), "--pos", p, "--max_kb_dist", str(max_kb)]
    m, f = os.path.join(d, "m.tsv"), os.path.join(d, "f.tsv")
    res = {}
    for name, extra in (("decay_out", ["--decay_out", m]), ("dmap_out_100kb", ["--dmap_out", m, "--dmap_window", "100000"]),
                        ("dmap_out_fit_100kb", ["--dmap_out", m, "--dmap_fit", f, "--dmap_window", "100000"])):
        t0 = time.perf_counter()
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, env={**os.environ, "NGSLD_TIMING": "1"})
        res[name + "_s"] = time.perf_counter() - t0
        if r.returncode != 0:
            res[name + "_error"] = r.stderr[-1000:]
        else:
            res[name + "_timing"] = [ln for ln in r.stderr.splitlines() if "LD decay" in ln]
    return res


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "dmap")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_maps(raw, chrs, pos, 100)
    with tempfile.TemporaryDirectory() as d:
        res["configs2_binary"] = binary_wall(raw, chrs, pos, d, 500, 100)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_maps(twin, chrs, pos, 100)
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "dmap_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
