"""The LD tree on one MI355X: the phases of ngsld_ld_tree on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window) and on its un-called twin (20 % monomorphic sites), at min_weight 0.5, 0.2 and 0.01 -- 0.01 is the floor with the
most edges, where a chunk's candidate list is longest and the reduce has most to read -- beside ngsld_clusters' union kernel and
ngsld_prune's edge extraction over the same records (at the same floors), and the tree plus five cuts beside five ngsld_clusters
calls at those five floors, all in the same process.  Each line is the best of three calls.

    python tools/tree_time.py [OUT_DIR]       (default profiles/tree; one JSON document, also printed)
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
STATS = ("pairs", "nodes", "edges", "merges", "clusters", "chunks", "rounds", "max_rounds", "displaced", "pairs_ms", "edges_ms",
         "reduce_ms", "finish_ms", "total_ms")


def five_cuts(w):
    """five floors from w up to 0.9, the first the tree's own"""
    return [w + (0.9 - w) * k / 4 for k in range(5)]


def timed_tree(raw, chrs, pos, max_kb, reps=3):
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
        eng.ld_tree(min_weight=0.5)                     # (warm caches and allocator)
        for w in FLOORS:
            sts, first = [], None
            for _ in range(reps):
                t0 = time.perf_counter()
                merges, st = eng.ld_tree(min_weight=w)
                st["wall_s"] = time.perf_counter() - t0
                sts.append(st)
                if first is None:
                    first = merges
                else:                                   # every call the same bits
                    assert all(merges[k].tobytes() == first[k].tobytes() for k in merges)
            best = min(sts, key=lambda s: s["total_ms"])
            entry = {k: best[k] for k in STATS}
            for k in ("pairs_ms", "edges_ms", "reduce_ms", "finish_ms", "total_ms"):
                entry[k + "_all"] = [round(s[k], 3) for s in sts]
            entry["edges_share_of_pairs"] = best["edges_ms"] / best["pairs_ms"]
            entry["reduce_share_of_pairs"] = best["reduce_ms"] / best["pairs_ms"]
            entry["call_over_pairs"] = best["total_ms"] / best["pairs_ms"]
            # the tree and five cuts beside five cluster calls at those floors
            cuts = five_cuts(w)
            t0 = time.perf_counter()
            eng.ld_tree(min_weight=w)
            ids = [eng.ld_tree_cut(t) for t in cuts]
            tree_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            t_cut = [eng.ld_tree_cut(t) for t in cuts]
            entry["five_cuts_ms"] = (time.perf_counter() - t0) * 1e3
            del t_cut
            t0 = time.perf_counter()
            csts = []
            for t, got in zip(cuts, ids):
                cl, _, cst = eng.clusters(min_weight=t, min_size=1)
                assert cl.tobytes() == got.tobytes()    # every cut is that call's ids
                csts.append(cst)
            clusters_s = time.perf_counter() - t0
            entry["tree_and_five_cuts_s"] = tree_s
            entry["five_cluster_calls_s"] = clusters_s
            entry["five_cluster_calls_over_tree_and_cuts"] = clusters_s / tree_s
            entry["clusters_at_the_floor"] = {k: csts[0][k] for k in ("union_ms", "pairs_ms", "total_ms", "edges", "clusters")}
            entry["clusters_same_edges_and_clusters"] = bool(csts[0]["edges"] == entry["edges"] and csts[0]["clusters"] == entry["clusters"])
            # the kernels that read the same 32 B a pair, same process, same box
            for _ in range(2 if w >= 0.1 else 1):       # (at a low floor pruning holds ~10^8 edges, ~1.6 GB of edge list: once)
                _, pst = eng.prune(labels, min_weight=w)
            entry["prune"] = {k: pst[k] for k in ("edges_ms", "pairs_ms", "total_ms", "edges")}
            entry["edges_ms_over_prune_edges_ms"] = best["edges_ms"] / pst["edges_ms"]
            entry["edges_ms_over_union_ms"] = best["edges_ms"] / csts[0]["union_ms"]
            out[f"min_weight_{w}"] = entry
    finally:
        eng.close()
    return out


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "tree")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(100_000, 2, max_gap=200)
    raw = synth.make_gl_numpy(100_000, 500, 2, depth=10.0)
    res["configs2"] = timed_tree(raw, chrs, pos, 100)
    del raw
    twin = synth.make_gl_numpy(100_000, 500, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_tree(twin, chrs, pos, 100)
    del twin
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "tree_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
