"""Linked pairs on one MI355X: the phases of ngsld_linked_pairs on BASELINE configs[2] at full size (100,000 sites x 500
individuals, 100 kb window) and on its un-called twin (20 % monomorphic sites), field 7 (r2) at floors 0.5, 0.2 and 0.01, records
only and records + text -- the pair phase, the count, scan and write kernels, the bytes handed to the sink, the whole call --
beside ngsld_prune's edge extraction and ngsld_clusters' union kernel at the same floors over the same records in the same
process.  Each line is the best of three calls.  The sink only counts: what a consumer does with the rows is its own time.

    python tools/linked_time.py [OUT_DIR] [--small] [--cli [--parent-cli=PATH]]
    (default OUT_DIR profiles/linked; one JSON document, also printed)
    --small: 20,000 sites instead of 100,000 (a quick look)
    --cli:   instead of the library's phases, the binary end to end on configs[2] as a file in /dev/shm: `--linked_out FILE` at
             floor 0.5 (no --out) against `--out /dev/null` -- the latter with the binary at PATH (a build of the parent commit)
             where --parent-cli is given, else with this tree's; twice each, both times written down (linked_cli.json)
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ngsld_amd import capi, shard, synth  # noqa: E402

FLOORS = (0.5, 0.2, 0.01)
KEYS = ("pairs", "rows", "text_bytes", "host_rows", "chunks", "pairs_ms", "count_ms", "scan_ms", "write_ms", "kernel_ms", "total_ms")


def linked_call(eng, labels_arr, floor, want):
    """One ngsld_linked_pairs call with a sink that only counts; (stats dict, batches, bytes the sink saw)."""
    p = capi.LinkedParams(C.sizeof(capi.LinkedParams), 7, float(floor), float("inf"), 0.0, 1, want)
    st = capi.LinkedStats()
    st.struct_size = C.sizeof(capi.LinkedStats)
    seen = [0, 0, 0]

    def sink(_user, bp):
        b = bp.contents
        seen[0] += 1
        seen[1] += b.n * ((8 + 32 + (40 if b.ext else 0)) if b.s1 else 0)
        seen[2] += b.text_len
        return 0

    t0 = time.perf_counter()
    rc = eng._L.ngsld_linked_pairs(eng._h, C.byref(p), labels_arr, capi.LINKED_FN(sink), None, C.byref(st))
    wall = time.perf_counter() - t0
    if rc != capi.OK:
        raise capi.NgsldError(rc, eng._L.ngsld_last_error(eng._h).decode())
    out = {k: getattr(st, k) for k in KEYS}
    out.update(wall_s=wall, batches=seen[0], record_bytes=seen[1], sink_text_bytes=seen[2])
    return out


def timed_linked(raw, chrs, pos, max_kb, reps=3):
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
        labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
        arr = (C.c_char_p * len(labels))(*[l.encode() for l in labels])
        linked_call(eng, arr, 0.5, capi.LINKED_RECORDS)  # (warm caches and allocator)
        for w in FLOORS:
            entry = {}
            for name, want in (("records", capi.LINKED_RECORDS), ("records_text", capi.LINKED_RECORDS | capi.LINKED_TEXT)):
                sts = [linked_call(eng, arr, w, want) for _ in range(reps)]
                assert len({(s["rows"], s["text_bytes"]) for s in sts}) == 1
                best = dict(min(sts, key=lambda s: s["total_ms"]))
                for k in ("pairs_ms", "count_ms", "scan_ms", "write_ms", "total_ms"):
                    best[k + "_all"] = [round(s[k], 3) for s in sts]
                best["call_over_pairs"] = best["total_ms"] / best["pairs_ms"]
                entry[name] = best
            # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2 if w >= 0.1 else 1):       # (at a low floor pruning holds ~10^8 edges, ~1.6 GB of edge list: once)
                _, pst = eng.prune(labels, min_weight=w)
            entry["prune"] = {k: pst[k] for k in ("edges_ms", "pairs_ms", "total_ms", "edges")}
            for _ in range(2):
                _, _, cst = eng.clusters(min_weight=w, min_size=1)
            entry["clusters"] = {k: cst[k] for k in ("union_ms", "pairs_ms", "total_ms", "edges")}
            entry["rows_equal_prune_edges"] = bool(entry["records"]["rows"] == pst["edges"])  # (one chromosome: no row across two)
            for name in ("records", "records_text"):
                entry[name]["kernels_over_prune_edges_ms"] = entry[name]["kernel_ms"] / pst["edges_ms"]
            out[f"min_weight_{w}"] = entry
    finally:
        eng.close()
    return out


def timed_cli(n_sites, parent_cli):
    import subprocess
    import tempfile
    out = {"n_sites": n_sites, "n_ind": 500, "table_binary": parent_cli or capi.CLI_PATH}
    with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
        chrs, pos = synth.make_positions(n_sites, 2, max_gap=200)
        g, p = os.path.join(d, "in.glf"), os.path.join(d, "in.pos")
        synth.make_gl_numpy(n_sites, 500, 2, depth=10.0).tofile(g)
        synth.write_pos(p, chrs, pos)
        base = ["--geno", g, "--n_ind", "500", "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "100", "--extend_out", "--n_threads",
                "16", "--verbose", "0"]
        runs = {"table_to_dev_null": [parent_cli or capi.CLI_PATH, *base, "--out", "/dev/null"],
                "linked_out_0.5": [capi.CLI_PATH, *base, "--linked_out", os.path.join(d, "linked.tsv"), "--linked_min_weight", "0.5"]}
        for name, argv in runs.items():
            times = []
            for _ in range(2):
                t0 = time.perf_counter()
                r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
                times.append(round(time.perf_counter() - t0, 3))
                assert r.returncode == 0, r.stderr[-2000:]
            out[name + "_s"] = times
        out["linked_file_bytes"] = os.path.getsize(os.path.join(d, "linked.tsv"))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    small = "--small" in sys.argv[1:]
    out_dir = args[0] if args else os.path.join(REPO, "profiles", "linked")
    os.makedirs(out_dir, exist_ok=True)
    n_sites = 20_000 if small else 100_000
    if "--cli" in sys.argv[1:]:
        parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent-cli=")), None)
        txt = json.dumps(timed_cli(n_sites, parent), indent=1)
        print(txt)
        with open(os.path.join(out_dir, "linked_cli.json"), "w") as fh:
            fh.write(txt + "\n")
        return
    res = {"n_sites": n_sites, "n_ind": 500, "max_kb_dist": 100}
    chrs, pos = synth.make_positions(n_sites, 2, max_gap=200)
    raw = synth.make_gl_numpy(n_sites, 500, 2, depth=10.0)
    res["configs2"] = timed_linked(raw, chrs, pos, 100)
    del raw
    twin = synth.make_gl_numpy(n_sites, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_linked(twin, chrs, pos, 100)
    del twin
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "linked_time_small.json" if small else "linked_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
