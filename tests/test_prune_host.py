"""LD pruning on the host, no GPU: ngsld_host_prune_graph against the restatement of prune_graph.pl (tests/prune_ref.py) on
seeded random graphs, the parallel rounds the device runs against the sequential rule, and ngsld_host_prune_label -- the
quantiser the device shares (ld_prune.h) -- against Python's own "%f" read back."""
import math
import struct

import numpy as np
import pytest

import prune_ref
from ngsld_amd import capi


def _graph(rng, kind):
    """(n, edges [(a, b, label)]) of one shape; at most one edge per pair."""
    n = int(rng.integers(1, 40))
    pairs = set()
    if kind == "chain":
        pairs = {(i, i + 1) for i in range(n - 1)}
    elif kind == "clique":
        n = min(n, 12)
        pairs = {(i, j) for i in range(n) for j in range(i + 1, n)}
    elif kind == "star":
        pairs = {(0, j) for j in range(1, n)}
    elif kind == "window":  # what a window of sites gives: every pair closer than k
        k = int(rng.integers(1, 6))
        pairs = {(i, j) for i in range(n) for j in range(i + 1, min(n, i + 1 + k))}
    else:  # random, isolated nodes likely
        m = int(rng.integers(0, 3 * n + 1))
        for _ in range(m):
            a, b = (int(x) for x in rng.integers(0, n, 2))
            if a != b:
                pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    lab_kind = rng.integers(0, 4)
    if lab_kind == 0:
        labels = [int(x) for x in rng.integers(0, 10001, len(pairs))]
    elif lab_kind == 1:  # ties everywhere
        labels = [int(x) for x in rng.integers(0, 3, len(pairs))]
    elif lab_kind == 2:  # all equal
        labels = [7] * len(pairs)
    else:  # zero labels among small ones
        labels = [int(x) * int(rng.integers(0, 2)) for x in rng.integers(0, 5, len(pairs))]
    return n, [(a, b, lab) for (a, b), lab in zip(pairs, labels)]


KINDS = ["random", "chain", "clique", "star", "window"]


def _check(n, edges, keep_heavy, rank):
    a = [e[0] for e in edges]
    b = [e[1] for e in edges]
    lab = [e[2] for e in edges]
    got, _ = capi.prune_graph(n, a, b, lab, keep_heavy=keep_heavy, rank=rank)
    want = prune_ref.prune_sequential(n, edges, keep_heavy, rank)
    assert set(np.nonzero(got)[0].tolist()) == want, (n, edges, keep_heavy, rank)


@pytest.mark.parametrize("keep_heavy", [False, True])
def test_host_pruner_equals_the_restatement(keep_heavy):
    """250 graphs per mode (chains, cliques, stars, windows, random with isolated nodes; ties, zero labels), random ranks."""
    rng = np.random.default_rng(11 + keep_heavy)
    for g in range(250):
        n, edges = _graph(rng, KINDS[g % len(KINDS)])
        rank = rng.permutation(n).tolist() if g % 2 else None
        _check(n, edges, keep_heavy, rank)


@pytest.mark.parametrize("keep_heavy", [False, True])
def test_host_pruner_with_negative_labels(keep_heavy):
    """Type 'e' on D / D': labels of both signs, weights that rise when a neighbour goes."""
    rng = np.random.default_rng(5 + keep_heavy)
    for g in range(100):
        n, edges = _graph(rng, KINDS[g % len(KINDS)])
        edges = [(a, b, int(rng.integers(-10000, 10001))) for a, b, _ in edges]
        _check(n, edges, keep_heavy, rng.permutation(n).tolist())


def test_parallel_rounds_equal_the_sequential_rule():
    """The confluence argument of PRUNE.md, checked: with labels >= 0, removing every strict local maximum of (weight desc,
    rank asc) at once, round after round, ends in the sequential rule's set -- on every graph."""
    rng = np.random.default_rng(3)
    for g in range(500):
        n, edges = _graph(rng, KINDS[g % len(KINDS)])
        rank = rng.permutation(n).tolist()
        assert prune_ref.prune_rounds(n, edges, rank) == prune_ref.prune_sequential(n, edges, False, rank), (n, edges, rank)


def test_rounds_do_not_hold_for_keep_heavy_or_negative_labels():
    """Why those two go to the host: a counterexample to each (the rule of the rounds is not theirs)."""
    # keep_heavy on a chain 0-1-2-3 with weights 1, 2, 2, 1 (labels 1, 1, 1): the script keeps 1 and drops 0, 2, then keeps 3
    edges = [(0, 1, 1), (1, 2, 1), (2, 3, 1)]
    assert prune_ref.prune_sequential(4, edges, True) == {0, 2}
    assert prune_ref.prune_rounds(4, edges) != {0, 2}
    # negative labels: removing a node can RAISE its neighbours' weights; among small random graphs some end elsewhere
    rng = np.random.default_rng(8)
    differ = 0
    for g in range(300):
        n, edges = _graph(rng, KINDS[g % len(KINDS)])
        edges = [(a, b, int(rng.integers(-5, 6))) for a, b, _ in edges]
        differ += prune_ref.prune_rounds(n, edges) != prune_ref.prune_sequential(n, edges)
    assert differ > 0


def test_host_pruner_refuses_bad_edges_and_overflow():
    with pytest.raises(capi.NgsldError):
        capi.prune_graph(3, [0], [0], [1])        # a loop
    with pytest.raises(capi.NgsldError):
        capi.prune_graph(3, [0], [3], [1])        # out of range
    with pytest.raises(capi.NgsldError) as e:
        capi.prune_graph(3, [0, 0], [1, 2], [2 ** 62, 2 ** 62])
    assert e.value.code == capi.ERR_UNSUPPORTED


def _want_label(x, prec=4, t="a"):
    if math.isnan(x) or math.isinf(x):
        return None
    w = float("%f" % x)
    if t == "a":
        w = abs(w)
    if t == "n":
        w = 1
    return int(w * 10 ** prec)


def _values(rng, n):
    """Random values of every kind the quantiser has a case for."""
    k = np.arange(-4096, 4097)
    out = [
        rng.random(n) * 2 - 1,                                 # r2 / D range
        rng.standard_normal(n) * 1e3,                          # large D'
        (rng.integers(-2 ** 20, 2 ** 20, n) / 128.0),          # k/128: exact ties at the sixth decimal
        (rng.integers(-10 ** 9, 10 ** 9, n) + 0.5) / 1e6,      # near-ties of the text
        np.ldexp(rng.random(n) + 1.0, rng.integers(-1074, 40, n)),  # every exponent, subnormals included
        k / 128.0, k * 5e-7, k * 1e-6,
    ]
    near = [2.0 ** 33]
    for v in near:
        out.append(np.array([np.nextafter(v, 0), v, np.nextafter(v, np.inf), -v, -np.nextafter(v, 0)]))
    out.append(np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 0.5e-6, 1.5e-6, 2.5e-6, -0.5e-6,
                         0.0000005, 0.9999995, 0.99999949999999, 1e-7, math.nan, -math.nan, math.inf, -math.inf]))
    return np.concatenate(out)


def test_label_equals_printed_value_read_back():
    """ngsld_host_prune_label(x) == int(abs(float('%f' % x)) * 10**prec) over ~3 million values."""
    rng = np.random.default_rng(2026)
    vals = _values(rng, 600_000)
    bad = []
    for x in vals.tolist():
        if _want_label(x) != capi.prune_label(x, 4, "a"):
            bad.append(x)
            if len(bad) > 5:
                break
    assert not bad, [(struct.pack("<d", x).hex(), x, _want_label(x), capi.prune_label(x)) for x in bad]
    assert len(vals) > 3_000_000


@pytest.mark.parametrize("prec,t", [(0, "a"), (2, "e"), (6, "e"), (9, "a"), (4, "n"), (15, "e")])
def test_label_precisions_and_types(prec, t):
    rng = np.random.default_rng(prec)
    for x in _values(rng, 3_000).tolist():
        if t == "e" and abs(x) * 10 ** prec >= 2 ** 62:
            continue
        try:
            got = capi.prune_label(x, prec, t)
        except capi.NgsldError as e:
            assert e.code == capi.ERR_UNSUPPORTED and abs(float("%f" % x)) * 10 ** prec >= 2 ** 62
            continue
        assert got == _want_label(x, prec, t), (x, prec, t)


def test_label_beyond_2_62_is_refused():
    with pytest.raises(capi.NgsldError) as e:
        capi.prune_label(2.0 ** 62 / 1e4, 4, "a")
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert capi.prune_label(2.0 ** 61 / 1e4, 4, "a") == int(float("%f" % (2.0 ** 61 / 1e4)) * 10 ** 4)


def test_tsv_restatement_filters():
    """prune_ref's edge filter on a hand-made TSV: NaN / inf weights, dist limit, non-finite dist, |w|, min_weight, subset."""
    hdr = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"
    rows = ["a:1\ta:2\t10\t0.5\t-0.3\t1.0\t0.25", "a:1\ta:3\t2000\t0.5\t0.3\t1.0\t0.5", "a:2\ta:3\t1990\t0.1\t0.1\t-nan\t-nan",
            "a:3\tb:1\tinf\t0.9\t0.9\t0.9\t0.9", "a:2\tb:1\tinf\t0.9\t0.9\t0.9\t0.9"]
    text = hdr + "\n".join(rows) + "\n"
    nodes, edges = prune_ref.tsv_graph(text)
    assert set(nodes) == {"a:1", "a:2", "a:3", "b:1"}
    assert edges == [("a:1", "a:2", 2500), ("a:1", "a:3", 5000)]
    _, edges = prune_ref.tsv_graph(text, field=5, max_kb_dist=1.995)
    assert edges == [("a:1", "a:2", 3000), ("a:2", "a:3", 1000)]
    _, edges = prune_ref.tsv_graph(text, field=5, weight_type="e", min_weight=-1.0)
    assert ("a:1", "a:2", -3000) in edges
    _, edges = prune_ref.tsv_graph(text, min_weight=0.3, weight_type="n")
    assert edges == [("a:1", "a:3", 10000)]
    nodes, edges = prune_ref.tsv_graph(text, subset={"a:1", "a:3"})
    assert set(nodes) == {"a:1", "a:3"} and edges == [("a:1", "a:3", 5000)]
    kept, excl = prune_ref.prune_tsv(text)
    assert excl == {"a:1"} and kept == {"a:2", "a:3", "b:1"}
