"""tests/partners_ref.py -- the rule of PARTNERS.md in plain Python -- held to hand-written tables, no GPU: a tie at the k-th
place broken by index, a tie between a left and a right partner, a value exactly on the floor, "-0.000000" against a signed
floor of 0, nan and inf rows, a row across chromosomes with and without a limit, a NaN maf, a query whose partners lie outside
it, k larger than any list, the range.  And the kernel's lock-free insertion (partners.hip, insert) as a simulation: its atomic
steps of several inserters interleaved at random, early exits on stale readings of the last slot included, against the sorted
top-k."""
import math
import random

import numpy as np
import pytest

import partners_ref

HEAD = ("site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\tsample_size\tmaf1\tmaf2\thap00\thap01\thap10\thap11\thap_maf1\thap_maf2\tchi2\t"
        "loglike\tnIter\n")
TAIL = "0.250000\t0.250000\t0.250000\t0.250000\t0.500000\t0.500000\t0.000000\t0.000000\t3"


def row(a, b, dist, e, d, dp, r2, maf1="0.200000", maf2="0.300000"):
    return f"s{a}\ts{b}\t{dist}\t{e}\t{d}\t{dp}\t{r2}\t8\t{maf1}\t{maf2}\t{TAIL}"


def run(rows, n, k, **kw):
    """rows: [(a, b, text of the row)] -> the rule's (rows, partner, value_micro) as lists."""
    text = HEAD + "".join(r + "\n" for _, _, r in rows)
    got = partners_ref.partners(text, [a for a, _, _ in rows], [b for _, b, _ in rows], n, k, **kw)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64 and got[2].dtype == np.int64
    assert got[1].shape == got[2].shape == (n, k)
    return [x.tolist() for x in got]


def r2_rows(pairs):
    return [(a, b, row(a, b, b - a, "0.100000", "0.010000", "0.300000", v)) for a, b, v in pairs]


def test_micro_strips_the_point():
    assert partners_ref.micro("0.500000") == 500000 and partners_ref.micro("-0.000001") == -1
    assert partners_ref.micro("-0.000000") == 0 and partners_ref.micro("2147.483647") == 2147483647
    assert partners_ref.micro("12345678901234567890.000001") == 12345678901234567890000001
    assert all(partners_ref.micro(t) is None for t in ("nan", "-nan", "inf", "-inf"))
    assert partners_ref.micro_text(-1) == "-0.000001" and partners_ref.micro_text(2147483647) == "2147.483647"
    assert partners_ref.micro_text(0) == "0.000000"


def test_a_tie_at_the_kth_place_is_broken_by_index_and_left_ties_with_right():
    # site 2: partners 0 and 4 tie at 0.9 (a left and a right one), 1 and 3 tie at 0.7; k = 3 keeps 1, the smaller index
    t = r2_rows([(0, 2, "0.900000"), (1, 2, "0.700000"), (2, 3, "0.700000"), (2, 4, "0.900000"), (2, 5, "0.600000")])
    rows, partner, value = run(t, 6, 3)
    assert rows == [1, 1, 5, 1, 1, 1]
    assert partner[2] == [0, 4, 1] and value[2] == [900000, 900000, 700000]
    assert partner[0] == [2, -1, -1] and value[0] == [900000, 0, 0]
    assert run(t, 6, 4)[1][2] == [0, 4, 1, 3] and run(t, 6, 1)[1][2] == [0]
    # k larger than any list: every list whole, in order
    rows, partner, value = run(t, 6, 64)
    assert partner[2][:6] == [0, 4, 1, 3, 5, -1] and value[2][:6] == [900000, 900000, 700000, 700000, 600000, 0]
    assert all(p[1] == -1 for s, p in enumerate(partner) if s != 2)


def test_the_floor_itself_passes_and_the_other_columns():
    t = [(0, 1, row(0, 1, 1, "0.100000", "0.010000", "0.300000", "0.500000")),    # on the floor
         (0, 2, row(0, 2, 2, "0.900000", "0.200000", "1.000000", "0.499999")),    # one unit below
         (1, 2, row(1, 2, 1, "0.100000", "-0.300000", "-1.000000", "0.500001"))]
    rows, partner, value = run(t, 3, 2)
    assert rows == [1, 2, 1] and partner == [[1, -1], [2, 0], [1, -1]] and value[1] == [500001, 500000]
    assert run(t, 3, 2, min_weight=0.500001)[0] == [0, 1, 1]
    assert run(t, 3, 2, field=4)[1] == [[2, -1], [-1, -1], [0, -1]]
    # D: absolute values rank -0.3 first; signed, it is below the floor, and with a floor of -1 it ranks last
    assert run(t, 3, 2, field=5, min_weight=0.2)[1:] == [[[2, -1], [2, -1], [1, 0]], [[200000, 0], [300000, 0], [300000, 200000]]]
    assert run(t, 3, 2, field=5, min_weight=0.2, abs_value=False)[1] == [[2, -1], [-1, -1], [0, -1]]
    rows, partner, value = run(t, 3, 2, field=5, min_weight=-1.0, abs_value=False)
    assert partner == [[2, 1], [0, 2], [0, 1]] and value == [[200000, 10000], [10000, -300000], [200000, -300000]]
    with pytest.raises(ValueError):
        run(t, 3, 2, field=3)
    with pytest.raises(ValueError):
        run(t, 3, 0)
    with pytest.raises(ValueError):
        run(t, 3, 65)


def test_minus_zero_nan_and_inf_rows():
    t = [(0, 1, row(0, 1, 1, "0.000000", "-0.000000", "-0.000000", "0.000000")),
         (0, 2, row(0, 2, 2, "-nan", "-nan", "nan", "-nan")),
         (1, 2, row(1, 2, 1, "0.100000", "inf", "-inf", "0.700000")),
         (1, 3, row(1, 3, 2, "0.100000", "-0.000001", "0.000001", "0.000000"))]
    # "-0.000000" is q = 0, which passes a signed floor of 0 and reads 0; a value one unit below does not pass
    rows, partner, value = run(t, 4, 2, field=5, min_weight=0.0, abs_value=False)
    assert rows == [1, 1, 0, 0] and partner[0] == [1, -1] and value[0] == [0, 0]
    assert run(t, 4, 2, field=5, min_weight=0.0)[0] == [1, 2, 0, 1]
    # nan and inf are never partner rows, whatever the floor
    assert run(t, 4, 2, field=5, min_weight=-math.inf, abs_value=False)[0] == [1, 2, 0, 1]
    assert run(t, 4, 2, field=6, min_weight=-math.inf, abs_value=False)[1] == [[1, -1], [3, 0], [-1, -1], [1, -1]]
    assert run(t, 4, 2, field=7, min_weight=-math.inf)[0] == [1, 3, 1, 1]
    assert run(t, 4, 2, field=4, min_weight=math.inf)[0] == [0, 0, 0, 0]


def test_across_chromosomes_a_nan_maf_and_a_query():
    t = [(0, 1, row(0, 1, 100, "0.100000", "0.100000", "0.100000", "0.900000")),
         (0, 2, row(0, 2, "inf", "0.100000", "0.100000", "0.100000", "0.800000")),              # across chromosomes
         (1, 2, row(1, 2, "inf", "0.100000", "0.100000", "0.100000", "0.700000", maf2="nan")),   # a NaN maf
         (0, 3, row(0, 3, 3000, "0.100000", "0.100000", "0.100000", "0.600000", maf2="0.049999"))]
    rows, partner, value = run(t, 4, 3)
    assert rows == [3, 1, 1, 1] and partner[0] == [1, 2, 3] and partner[2] == [0, -1, -1]
    # a finite limit, however large, drops the rows across chromosomes; one inside the chromosome drops the far row
    assert run(t, 4, 3, max_kb_dist=1e9)[1][0] == [1, 3, -1]
    assert run(t, 4, 3, max_kb_dist=3.0)[1][0] == [1, 3, -1] and run(t, 4, 3, max_kb_dist=2.999)[1][0] == [1, -1, -1]
    assert run(t, 4, 3, min_maf=0.05)[1][0] == [1, 2, -1] and run(t, 4, 3, min_maf=0.049999)[1][0] == [1, 2, 3]
    # a query: sites 0 and 3 collect, their partners 1 and 2 lie outside it and collect nothing
    rows, partner, value = run(t, 4, 3, query=[1, 0, 0, 1])
    assert rows == [3, 0, 0, 1] and partner == [[1, 2, 3], [-1] * 3, [-1] * 3, [0, -1, -1]]
    assert run(t, 4, 3, query=[0, 0, 0, 0])[0] == [0, 0, 0, 0]
    # a table without the extended columns takes the sites' maf from a map
    plain = HEAD + "".join("\t".join(r.split("\t")[:7]) + "\n" for _, _, r in t)
    maf = {"s0": 0.2, "s1": 0.3, "s2": math.nan, "s3": 0.049999}
    got = partners_ref.partners(plain, [0, 0, 1, 0], [1, 2, 2, 3], 4, 3, maf=maf)
    assert got[1][0].tolist() == [1, 3, -1] and got[0].tolist() == [2, 1, 0, 1]
    with pytest.raises(ValueError):
        partners_ref.partners(plain, [0, 0, 1, 0], [1, 2, 2, 3], 4, 3)


def test_the_range():
    ok = [(0, 1, row(0, 1, 1, "0.100000", "0.100000", "2147.483647", "0.500000")),
          (0, 2, row(0, 2, 2, "0.100000", "0.100000", "-2147.483647", "0.500000"))]
    rows, partner, value = run(ok, 3, 2, field=6)
    assert partner[0] == [1, 2] and value[0] == [2147483647, 2147483647]
    assert run(ok, 3, 2, field=6, abs_value=False, min_weight=-math.inf)[2][0] == [2147483647, -2147483647]
    for bad in ("2147.483648", "-2147.483648", "1" + "0" * 300 + ".000000"):
        t = ok + [(1, 2, row(1, 2, 1, "0.100000", "0.100000", bad, "0.500000"))]
        with pytest.raises(partners_ref.RangeError) as e:
            run(t, 3, 2, field=6)
        assert e.value.pair == (1, 2)
        with pytest.raises(partners_ref.RangeError):  # (whatever the floor)
            run(t, 3, 2, field=6, min_weight=math.inf)
        assert run(t, 3, 2, field=7)[0] == [2, 2, 2]           # the column is not chosen
        assert run(t, 3, 2, field=6, min_maf=0.25)[0] == [0, 0, 0]  # the maf filter drops the row first


def test_the_file():
    t = r2_rows([(0, 2, "0.900000"), (1, 2, "0.700000")])
    _, partner, value = run(t, 3, 2)
    assert partners_ref.partners_file(partner, value, ["a:1", "a:2", "a:3"]) == (
        "site\trank\tpartner\tr2\na:1\t1\ta:3\t0.900000\na:2\t1\ta:3\t0.700000\na:3\t1\ta:1\t0.900000\na:3\t2\ta:2\t0.700000\n")
    assert partners_ref.partners_file(partner, value, ["1", "2", "3"], field=6).startswith("site\trank\tpartner\tDp\n1\t1\t3\t")


# ---- the insertion of partners.hip, interleaved ----
class Inserter:
    """One call of insert(slot, k, key) as its atomic steps: the first reading of the last slot, then atomicMax on slot j and a
    fresh reading of the last slot in turn.  A reading may be stale: any value the last slot has held so far."""

    def __init__(self, key):
        self.key, self.carry, self.j, self.state = key, key, 0, "first"

    def step(self, slots, last_history, rng):
        k = len(slots)
        if self.state in ("first", "peek"):
            seen = rng.choice(last_history) if rng.random() < 0.5 else slots[k - 1]
            self.state = "done" if self.carry <= seen else "max"
            return
        old = slots[self.j]
        slots[self.j] = max(old, self.carry)       # atomicMax
        self.carry = min(old, self.carry)
        if self.j == k - 1:
            last_history.append(slots[k - 1])
        self.j += 1
        self.state = "done" if (self.carry == 0 or self.j == k) else "peek"


def test_interleaved_insertions_give_the_sorted_top_k():
    rng = random.Random(20)
    for trial in range(3000):
        k = rng.randint(1, 6)
        keys = rng.sample(range(1, 200), rng.randint(0, 30))  # distinct, never 0
        slots, history = [0] * k, [0]
        waiting, flying = list(keys), []
        while waiting or flying:
            while waiting and len(flying) < 8:
                flying.append(Inserter(waiting.pop()))
            ins = rng.choice(flying)
            ins.step(slots, history, rng)
            if ins.state == "done":
                flying.remove(ins)
        want = sorted(keys, reverse=True)[:k]
        assert slots == want + [0] * (k - len(want)), (trial, k, keys, slots)


def test_the_key_orders_as_the_rule():
    """key = (q + 2^31) << 32 | (2^32 - 1 - partner): never 0 for |q| < 2^31, and its unsigned order is (q descending, partner
    ascending)."""
    key = lambda q, p: ((q + (1 << 31)) << 32) | (0xFFFFFFFF - p)  # noqa: E731
    qs = [-(1 << 31) + 1, -1, 0, 1, 500000, (1 << 31) - 1]
    ps = [0, 1, 299, 0xFFFFFFFE]
    items = [(q, p) for q in qs for p in ps]
    assert all(0 < key(q, p) < 1 << 64 for q, p in items)
    assert sorted(items, key=lambda x: -key(*x)) == sorted(items, key=lambda x: (-x[0], x[1]))
    for q, p in items:
        assert ((key(q, p) >> 32) - (1 << 31), 0xFFFFFFFF - (key(q, p) & 0xFFFFFFFF)) == (q, p)
