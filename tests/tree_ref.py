"""Plain Python restatement of the LD tree (TREE.md rules 2-5) over the TSV text ngsLD writes -- the yardstick of ngsld_ld_tree,
the way cluster_ref.py is of ngsld_clusters, whose nodes and edges (rule 1, cluster_ref.tsv_edges) it takes as they are.

* order: edge e comes before edge f iff q_e > q_f, or the q are equal and s1_e < s1_f, or those are equal too and s2_e < s2_f
  (`sorted` on (-q, s1, s2));
* forest: the edges in that order, an edge is kept iff its two ends lie in different trees so far (a dictionary union-find);
* merges: the kept edges in that order, numbered from 1, each with s1, s2, q, dist = position of s2 - position of s1 (the
  positions are the labels' part after the last ":"), left and right = the clusters that held s1 and s2 before the merge
  (-(site index + 1) for a single site, else the number of the merge that made it), size, first and last of the merged cluster;
* cut(t): the merges with q / 10^6 >= t as doubles -- a prefix -- united, the components numbered 1, 2, ... in increasing order
  of their smallest site index, singletons included, 0 for a site that is not a node.
"""
from __future__ import annotations

import cluster_ref
from cluster_ref import MICRO, micro_text, position

HEADER = "merge\tsite1\tsite2\tweight\tdist\tleft\tright\tsize\tfirst\tlast"


def order(edges):
    """The edges (s1, s2, q) in rule order."""
    return sorted(edges, key=lambda e: (-e[2], e[0], e[1]))


def _find(parent, v):
    while parent[v] != v:
        parent[v] = parent[parent[v]]
        v = parent[v]
    return v


def forest(edges):
    """The maximum spanning forest of the edges (s1, s2, q) under the rule order, as the list of its edges in that order."""
    parent, kept = {}, []
    for e in order(edges):
        parent.setdefault(e[0], e[0])
        parent.setdefault(e[1], e[1])
        a, b = _find(parent, e[0]), _find(parent, e[1])
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.append(e)
    return kept


def forest_in_parts(parts):
    """The forest built part by part: forest so far + the next part of the edges, reduced; what a chunked run keeps."""
    kept = []
    for part in parts:
        kept = forest(kept + list(part))
    return kept


def merges(edges, sites: list[str] | None = None) -> list[dict]:
    """The merges of the edge set: one dict per forest edge, in rule order (dist is None without labels)."""
    parent, name, size, last, rows = {}, {}, {}, {}, []
    for s1, s2, q in forest(edges):
        for s in (s1, s2):
            if s not in parent:
                parent[s], name[s], size[s], last[s] = s, -(s + 1), 1, s
        a, b = _find(parent, s1), _find(parent, s2)
        assert a != b
        lo, hi = min(a, b), max(a, b)
        row = dict(s1=s1, s2=s2, q=q, dist=None if sites is None else position(sites[s2]) - position(sites[s1]),
                   left=name[a], right=name[b])
        parent[hi] = lo
        size[lo] += size[hi]
        last[lo] = max(last[lo], last[hi])
        name[lo] = len(rows) + 1
        row.update(size=size[lo], first=lo, last=last[lo])
        rows.append(row)
    return rows


def tree(text: str, sites: list[str], **kw) -> tuple[set, list[dict]]:
    """(nodes, merges) of an ngsLD TSV; kw as cluster_ref.tsv_edges takes them (min_weight is the tree's floor)."""
    kw.setdefault("min_weight", 0.1)
    nodes, edges = cluster_ref.tsv_edges(text, sites, **kw)
    return nodes, merges(edges, sites)


def cut(nodes, rows: list[dict], n_sites: int, t: float) -> list[int]:
    """Every site's cluster id at the floor t, from the merges alone."""
    parent = {s: s for s in nodes}
    live = [r["q"] / MICRO >= t for r in rows]
    assert live == sorted(live, reverse=True), "the merges at or above a floor are a prefix"
    for r, on in zip(rows, live):
        if on:
            a, b = _find(parent, r["s1"]), _find(parent, r["s2"])
            parent[max(a, b)] = min(a, b)
    ids, seen = [0] * n_sites, {}
    for s in sorted(nodes):
        ids[s] = seen.setdefault(_find(parent, s), len(seen) + 1)
    return ids


def tree_file(rows: list[dict], names: list[str]) -> str:
    """The --tree_out file: header, then one line per merge (names: how a site is written)."""
    out = [HEADER]
    for k, r in enumerate(rows):
        out.append("\t".join([str(k + 1), names[r["s1"]], names[r["s2"]], micro_text(r["q"]), str(r["dist"]), str(r["left"]),
                              str(r["right"]), str(r["size"]), names[r["first"]], names[r["last"]]]))
    return "\n".join(out) + "\n"


def cuts_file(columns: list[list[int]], floors: list[str], names: list[str]) -> str:
    """The --tree_cut_out file: header (the floors as typed), then one line per site with its cluster at every floor or NA."""
    out = ["\t".join(["site", *floors])]
    for s, lab in enumerate(names):
        out.append("\t".join([lab, *("NA" if col[s] == 0 else str(col[s]) for col in columns)]))
    return "\n".join(out) + "\n"
