"""tests/tree_ref.py, the plain-Python restatement of the LD tree (TREE.md), held to hand-worked tables, to cluster_ref at every
cut, and to itself when the edges arrive in parts; then the rounds tree.hip runs -- best q, best key, hook, flatten -- restated
over Python lists and held to the same forest and to the bound on the rounds.  No GPU."""
import math
import random

import cluster_ref
import tree_ref


def _tsv(rows):
    """site1 site2 dist r2_ExpG D Dp r2 -- the r2 column is the one the defaults read."""
    return "".join(f"c:{a}\tc:{b}\t{b - a}\t0.000000\t0.000000\t0.000000\t{w}\n" for a, b, w in rows)


SITES = [f"c:{k}" for k in range(8)]


def test_a_hand_worked_tree():
    #   0 -0.9- 1 -0.5- 2      3 -0.7- 4       5 (in a pair below the floor: a node, a singleton)   7: in no row
    #   0 -0.4- 2 closes a cycle and is dropped; 2 -0.2- 3 joins the two trees last
    text = _tsv([(0, 1, "0.900000"), (1, 2, "0.500000"), (0, 2, "0.400000"), (3, 4, "0.700000"), (2, 3, "0.200000"),
                 (5, 6, "0.050000")])
    nodes, rows = tree_ref.tree(text, SITES)
    assert nodes == {0, 1, 2, 3, 4, 5, 6}
    assert [(r["s1"], r["s2"], r["q"]) for r in rows] == [(0, 1, 900000), (3, 4, 700000), (1, 2, 500000), (2, 3, 200000)]
    assert [(r["left"], r["right"]) for r in rows] == [(-1, -2), (-4, -5), (1, -3), (3, 2)]
    assert [(r["size"], r["first"], r["last"], r["dist"]) for r in rows] == [(2, 0, 1, 1), (2, 3, 4, 1), (3, 0, 2, 1), (5, 0, 4, 1)]
    assert len(rows) == len(nodes) - 3  # (clusters at the floor: {0..4}, {5}, {6})
    assert tree_ref.cut(nodes, rows, 8, 0.1) == [1, 1, 1, 1, 1, 2, 3, 0]
    assert tree_ref.cut(nodes, rows, 8, 0.5) == [1, 1, 1, 2, 2, 3, 4, 0]
    assert tree_ref.cut(nodes, rows, 8, 0.500001) == [1, 1, 2, 3, 3, 4, 5, 0]
    assert tree_ref.cut(nodes, rows, 8, 0.95) == [1, 2, 3, 4, 5, 6, 7, 0]
    assert tree_ref.tree_file(rows[:1], SITES) == tree_ref.HEADER + "\n1\tc:0\tc:1\t0.900000\t1\t-1\t-2\t2\tc:0\tc:1\n"
    assert tree_ref.cuts_file([[1, 0], [2, 0]], ["0.5", ".2"], ["a", "b"]) == "site\t0.5\t.2\na\t1\t2\nb\tNA\tNA\n"


def test_equal_weights_go_by_the_sites():
    # a triangle and a square of one weight: which edges stay is decided by (s1, s2) alone
    text = _tsv([(1, 2, "0.500000"), (0, 2, "0.500000"), (0, 1, "0.500000"),
                 (3, 4, "0.300000"), (4, 5, "0.300000"), (5, 6, "0.300000"), (3, 6, "0.300000")])
    _, rows = tree_ref.tree(text, SITES)
    assert [(r["s1"], r["s2"]) for r in rows] == [(0, 1), (0, 2), (3, 4), (3, 6), (4, 5)]
    assert [(r["left"], r["right"]) for r in rows] == [(-1, -2), (1, -3), (-4, -5), (3, -7), (4, -6)]
    # the same rows in another order: the same merges
    lines = text.splitlines(keepends=True)
    assert tree_ref.tree("".join(reversed(lines)), SITES)[1] == rows
    # signed: -0.6 is below every floor >= 0; absolute, it is the heaviest edge
    text = _tsv([(0, 1, "-0.600000"), (1, 2, "0.200000")])
    assert [r["q"] for r in tree_ref.tree(text, SITES)[1]] == [600000, 200000]
    assert [r["q"] for r in tree_ref.tree(text, SITES, abs_value=False)[1]] == [200000]
    assert [r["q"] for r in tree_ref.tree(text, SITES, abs_value=False, min_weight=-1.0)[1]] == [200000, -600000]


def _graph(rng):
    """A random graph of 5..40 sites with many equal weights, as TSV rows; some pairs lie below the floor 0.1."""
    n = rng.randint(5, 40)
    sites = [f"c:{k * 10}" for k in range(n)]
    weights = [rng.randint(0, 12) * 50000 + rng.choice((0, 0, 0, 1)) for _ in range(rng.randint(2, 6))]
    rows = []
    for a in range(n):
        for b in range(a + 1, n):
            if rng.random() < rng.choice((0.1, 0.3)):
                rows.append(f"{sites[a]}\t{sites[b]}\t{(b - a) * 10}\t0.000000\t0.000000\t0.000000\t{cluster_ref.micro_text(rng.choice(weights))}\n")
    return sites, "".join(rows)


GRAPHS = 500


def test_every_cut_gives_the_clusters_of_that_floor():
    rng = random.Random(20)
    seen_ties = 0
    for _ in range(GRAPHS):
        sites, text = _graph(rng)
        nodes, rows = tree_ref.tree(text, sites)
        qs = [r["q"] for r in rows]
        seen_ties += len(qs) - len(set(qs))
        assert qs == sorted(qs, reverse=True)
        ids_floor, table = cluster_ref.clusters(text, sites, min_size=1, min_weight=0.1)
        assert len(rows) == len(nodes) - len(table)
        floors = sorted({0.1, 1.0, *(q / 1e6 for q in qs), *(q / 1e6 + 1e-6 for q in qs[:3])})
        for t in floors:
            assert tree_ref.cut(nodes, rows, len(sites), t) == cluster_ref.clusters(text, sites, min_size=1, min_weight=t)[0], t
        assert tree_ref.cut(nodes, rows, len(sites), 0.1) == ids_floor
    assert seen_ties > GRAPHS  # (the graphs do hold equal weights)


def test_the_forest_built_in_parts_is_the_forest_of_the_whole():
    rng = random.Random(21)
    displaced = 0
    for _ in range(GRAPHS):
        sites, text = _graph(rng)
        _, edges = cluster_ref.tsv_edges(text, sites, min_weight=0.1)
        whole = tree_ref.forest(edges)
        rng.shuffle(edges)
        cuts = sorted(rng.randint(0, len(edges)) for _ in range(rng.randint(1, 6)))
        parts = [edges[a:b] for a, b in zip([0, *cuts], [*cuts, len(edges)])]
        assert tree_ref.forest_in_parts(parts) == whole
        kept = []
        for part in parts:  # (an edge kept after one part and gone after a later one: the reduce does replace edges)
            new = tree_ref.forest(kept + part)
            displaced += len(set(kept) - set(new))
            kept = new
    assert displaced > GRAPHS


# ---- the device's rounds (tree.hip), restated ----
BIAS = 1 << 38


def _boruvka(n, edges):
    """best q (max), best key (min among that q), hook (the chooser under the other; a mutual choice: larger under smaller),
    flatten -- until a round keeps nothing.  Returns (the kept edges, rounds)."""
    comp, kept, rounds = list(range(n)), [], 0
    while True:
        rounds += 1
        best_q, best_key, hook = [0] * n, [(1 << 64) - 1] * n, list(range(n))
        for s1, s2, q in edges:
            a, b = comp[s1], comp[s2]
            if a != b:
                best_q[a], best_q[b] = max(best_q[a], q + BIAS), max(best_q[b], q + BIAS)
        for s1, s2, q in edges:
            a, b = comp[s1], comp[s2]
            if a != b:
                for r in (a, b):
                    if best_q[r] == q + BIAS:
                        best_key[r] = min(best_key[r], s1 << 32 | s2)
        new = 0
        for s1, s2, q in edges:
            a, b = comp[s1], comp[s2]
            if a == b:
                continue
            by_a, by_b = ((best_q[r], best_key[r]) == (q + BIAS, s1 << 32 | s2) for r in (a, b))
            if by_a and by_b:
                hook[max(a, b)] = min(a, b)
            elif by_a:
                hook[a] = b
            elif by_b:
                hook[b] = a
            if by_a or by_b:
                kept.append((s1, s2, q))
                new += 1
        for v in range(n):
            r = comp[v]
            while hook[r] != r:
                r = hook[r]
            comp[v] = r
        if new == 0:
            return kept, rounds


def test_the_rounds_of_the_device_keep_the_same_forest():
    rng = random.Random(22)
    for _ in range(GRAPHS):
        sites, text = _graph(rng)
        _, edges = cluster_ref.tsv_edges(text, sites, min_weight=0.1)
        rng.shuffle(edges)
        kept, rounds = _boruvka(len(sites), edges)
        assert tree_ref.order(kept) == tree_ref.forest(edges)
        assert rounds <= math.ceil(math.log2(len(sites))) + 1
    # a path whose weights rise along it: every site chooses the edge to its right, one chain of hooks, two rounds
    path = [(k, k + 1, 100000 + k) for k in range(999)]
    kept, rounds = _boruvka(1000, path)
    assert sorted(kept) == path and rounds == 2
