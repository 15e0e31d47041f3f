"""LD clusters on one MI355X: the phases of ngsld_clusters on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window) and on its un-called twin (20 % monomorphic sites), at min_weight 0.5, 0.2 and 0.01 -- 0.01 is the
floor with the most edges, where an edge list is largest and the roots are contended most -- beside ngsld_prune's edge extraction (at the
same floors) and ngsld_site_ld's kernel over the same records in the same process.  Each line is the best of three calls.

    python tools/cluster_time.py [OUT_DIR]       (default profiles/clusters; one JSON document, also printed)
"""
from __future__ import annotations

import json
import os
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ngsld_amd import capi, shard, synth  # noqa: E402

FLOORS = (0.5, 0.2, 0.01)


def timed_clusters(raw, chrs, pos, max_kb, reps=3):
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
        eng.clusters()                                  # (warm caches and allocator)
        for w in FLOORS:
            sts, first = [], None
            for _ in range(reps):
                t0 = time.perf_counter()
                ids, table, st = eng.clusters(min_weight=w, min_size=1)
                st["wall_s"] = time.perf_counter() - t0
                sts.append(st)
                if first is None:
                    first = (ids, table)
                else:                                   # every call the same bits
                    assert ids.tobytes() == first[0].tobytes()
                    assert all(table[k].tobytes() == first[1][k].tobytes() for k in table)
            best = min(sts, key=lambda s: s["total_ms"])
            entry = {k: best[k] for k in ("pairs", "nodes", "edges", "clusters", "clusters_multi", "largest", "chunks", "union_launches",
                                          "pairs_ms", "union_ms", "finish_ms", "total_ms")}
            for k in ("pairs_ms", "union_ms", "finish_ms", "total_ms"):
                entry[k + "_all"] = [round(s[k], 3) for s in sts]
            entry["union_share_of_pairs"] = best["union_ms"] / best["pairs_ms"]
            entry["call_over_pairs"] = best["total_ms"] / best["pairs_ms"]
            ids, table = first
            big = int(table["size"].argmax())
            entry["largest_cluster"] = {k: (float(table[k][big]) if k in ("mean", "density") else int(table[k][big])) for k in table}
            # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2 if w >= 0.1 else 1):       # (at a low floor pruning holds ~10^8 edges, ~1.6 GB of edge list: once)
                _, pst = eng.prune(labels, min_weight=w)
            entry["prune"] = {k: pst[k] for k in ("edges_ms", "pairs_ms", "total_ms", "edges", "kept")}
            entry["prune_same_edges_and_kept_at_least_clusters"] = bool(pst["edges"] == entry["edges"] and pst["kept"] >= entry["clusters"])
            entry["union_ms_over_prune_edges_ms"] = best["union_ms"] / pst["edges_ms"]
            out[f"min_weight_{w}"] = entry
        for _ in range(2):
            _, sst = eng.site_ld()
        out["site_ld_r2"] = {k: sst[k] for k in ("site_ms", "pairs_ms", "total_ms", "lds")}
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "clusters")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_clusters(raw, chrs, pos, 100)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_clusters(twin, chrs, pos, 100)
    del twin
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "cluster_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
