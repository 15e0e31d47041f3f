"""Plain Python restatement of the reference's LD pruner (scripts/prune_graph.pl v1.2.2, its prune_graph_idx path) over the
TSV text ngsLD writes -- the yardstick of ngsld_prune, the way oracle/ restates ngsLD.  PRUNE.md has the rule.

* nodes: both ends of every row (only labels in the subset, when one is given);
* edge filter, per row, in the script's order: the weight field read back with float(); NaN / inf skipped; a dist above
  max_kb_dist * 1000 skipped (a dist that is not finite is never an edge: the script refuses such a file); |w| for type 'a';
  w < min_weight skipped; both ends in the subset; 1 for type 'n'; label = int(w * 10**precision);
* until the heaviest node weighs <= 0: remove it (or, keep_heavy, all its neighbours), ties to lc(label), then the label's
  bytes, then the site order.
"""
from __future__ import annotations

import math


def tsv_graph(text: str, field: int = 7, max_kb_dist: float = math.inf, min_weight: float = 0.0, weight_type: str = "a",
              subset=None, precision: int = 4):
    """(nodes: {label: first appearance}, edges: [(label1, label2, int label)]) of an ngsLD TSV (header line included)."""
    nodes: dict[str, int] = {}
    edges = []
    max_dist = max_kb_dist * 1000
    scale = 10 ** precision
    for line in text.splitlines():
        if not line or line.startswith("site1\t"):
            continue
        f = line.split("\t")
        l1, l2 = f[0], f[1]
        for lab in (l1, l2):
            if subset is None or lab in subset:
                nodes.setdefault(lab, len(nodes))
        w = float(f[field - 1])
        if math.isnan(w) or math.isinf(w):
            continue
        dist = float(f[2])
        if not math.isfinite(dist) or dist > max_dist:
            continue
        if weight_type == "a":
            w = abs(w)
        if w < min_weight:
            continue
        if subset is not None and not (l1 in subset and l2 in subset):
            continue
        if weight_type == "n":
            w = 1
        edges.append((l1, l2, int(w * scale)))
    return nodes, edges


def prune_sequential(n: int, edges, keep_heavy: bool = False, rank=None) -> set[int]:
    """The script's loop on nodes 0 .. n-1 and edges (a, b, label); returns the excluded nodes.  Ties: the lower rank[]."""
    rank = list(range(n)) if rank is None else list(rank)
    adj: list[dict[int, int]] = [dict() for _ in range(n)]
    for a, b, lab in edges:
        adj[a][b] = lab
        adj[b][a] = lab
    w = {v: sum(adj[v].values()) for v in range(n)}
    live = set(range(n))
    excluded: set[int] = set()

    def remove(v):
        live.discard(v)
        excluded.add(v)
        for u, lab in adj[v].items():
            if u in live:
                w[u] -= lab
        del w[v]

    while w:
        top = min(w, key=lambda v: (-w[v], rank[v]))
        if w[top] <= 0:
            break
        if keep_heavy:
            for u in [u for u in adj[top] if u in live]:
                remove(u)
        else:
            remove(top)
    return excluded


def prune_rounds(n: int, edges, rank=None) -> set[int]:
    """The device's rule (labels >= 0, the heaviest removed): in rounds, every live node of weight > 0 whose (weight desc,
    rank asc) beats all its live neighbours goes at once.  Returns the excluded nodes."""
    rank = list(range(n)) if rank is None else list(rank)
    adj: list[dict[int, int]] = [dict() for _ in range(n)]
    for a, b, lab in edges:
        adj[a][b] = lab
        adj[b][a] = lab
    w = [sum(adj[v].values()) for v in range(n)]
    live = [True] * n
    excluded: set[int] = set()
    while True:
        key = lambda v: (w[v], -rank[v])  # noqa: E731
        marked = [v for v in range(n) if live[v] and w[v] > 0 and all(key(v) > key(u) for u in adj[v] if live[u])]
        if not marked:
            return excluded
        for v in marked:
            live[v] = False
            excluded.add(v)
            for u, lab in adj[v].items():
                w[u] -= lab


def label_order(labels: list[str]) -> list[int]:
    """rank of every label: lc() as Perl's (ASCII letters only), then the bytes, then the position."""
    keyed = sorted(range(len(labels)), key=lambda i: (labels[i].encode().lower(), labels[i].encode(), i))
    rank = [0] * len(labels)
    for r, i in enumerate(keyed):
        rank[i] = r
    return rank


def prune_tsv_counts(text: str, keep_heavy: bool = False, **kw) -> tuple[set[str], set[str], int, int]:
    """(kept, excluded, nodes, edges) of an ngsLD TSV: prune_tsv's sets, and how many nodes and edges (rows that pass the edge
    filter: a pair is one row of the table) the graph they were pruned from has."""
    nodes, edges = tsv_graph(text, **kw)
    names = list(nodes)
    index = {lab: i for i, lab in enumerate(names)}
    excl = prune_sequential(len(names), [(index[a], index[b], lab) for a, b, lab in edges], keep_heavy, label_order(names))
    return {names[i] for i in range(len(names)) if i not in excl}, {names[i] for i in excl}, len(names), len(edges)


def prune_tsv(text: str, keep_heavy: bool = False, **kw) -> tuple[set[str], set[str]]:
    """(kept, excluded) labels of an ngsLD TSV, as prune_graph.pl prints them (as sets)."""
    return prune_tsv_counts(text, keep_heavy, **kw)[:2]
