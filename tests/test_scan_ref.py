"""tests/scan_ref.py -- the rule of SCAN.md in plain Python -- held to hand-worked tables, and its range decomposition (a counted
row belongs to the windows of a contiguous range of centre sites, per class) held to the definition applied window by window on
random layouts: repeated positions, several chromosomes, half windows from 0 to beyond the chromosome.  No GPU, no engine."""
import math
import random

import scan_ref


def _row(a, b, dist, r2, d="0.010000", dp="0.500000", expg=None):
    return "\t".join([a, b, dist, expg if expg is not None else r2, d, dp, r2])


# one chromosome of five sites 100 bp apart; r2 of the pair (i, j) prints as 0.(i+1)(j+1)0000
SITES5 = [f"c:{100 * (k + 1)}" for k in range(5)]
Q5 = {(i, j): (10 * (i + 1) + (j + 1)) * 10000 for i in range(5) for j in range(i + 1, 5)}
TEXT5 = "\n".join(_row(SITES5[i], SITES5[j], str(100 * (j - i)), scan_ref.micro_text(q)) for (i, j), q in Q5.items()) + "\n"


def test_five_sites_half_window_150():
    """Windows [0,1] [0,2] [1,3] [2,4] [3,4]: the rows 200 bp and more apart are in no window."""
    res = scan_ref.scan(TEXT5, SITES5, 150)
    assert res["win_first"] == [0, 0, 1, 2, 3] and res["win_last"] == [1, 2, 3, 4, 4]
    assert res["n_ll"] == [0, 1, 1, 1, 1] and res["n_rr"] == [0, 0, 0, 0, 0] and res["n_lr"] == [1, 2, 2, 2, 0]
    assert res["sum_ll_r2"] == [0, 120000, 230000, 340000, 450000]
    assert res["sum_rr_r2"] == [0, 0, 0, 0, 0]
    assert res["sum_lr_r2"] == [120000, 360000, 580000, 800000, 0]
    assert res["zns_r2"] == [0.12, 480000 / 3e6, 810000 / 3e6, 1140000 / 3e6, 0.45]
    # omega: no row inside a flank at site 0, no row across at site 4
    assert res["omega_r2"] == [None, 240000 / 360000, 460000 / 580000, 680000 / 800000, None]


def test_five_sites_half_window_250_has_all_three_classes():
    res = scan_ref.scan(TEXT5, SITES5, 250)
    assert res["win_first"] == [0, 0, 0, 1, 2] and res["win_last"] == [2, 3, 4, 4, 4]
    # site 2 sees the whole table: LL (0,1) (0,2) (1,2); RR (3,4); LR the other six
    assert (res["n_ll"][2], res["n_rr"][2], res["n_lr"][2]) == (3, 1, 6)
    assert (res["sum_ll_r2"][2], res["sum_rr_r2"][2], res["sum_lr_r2"][2]) == (480000, 450000, 1470000)
    assert res["zns_r2"][2] == 2400000 / 10e6
    assert res["omega_r2"][2] == (930000 * 6) / (4 * 1470000)
    # site 1, window [0,3]: LL (0,1); RR (2,3); LR (0,2) (0,3) (1,2) (1,3)
    assert (res["n_ll"][1], res["n_rr"][1], res["n_lr"][1]) == (1, 1, 4)
    assert (res["sum_ll_r2"][1], res["sum_rr_r2"][1], res["sum_lr_r2"][1]) == (120000, 340000, 130000 + 140000 + 230000 + 240000)
    assert scan_ref.scan(TEXT5, SITES5, 250, brute=True) == res


def test_half_window_beyond_the_chromosome():
    res = scan_ref.scan(TEXT5, SITES5, 10 ** 9)
    assert res["win_first"] == [0] * 5 and res["win_last"] == [4] * 5
    assert [a + b + c for a, b, c in zip(res["n_ll"], res["n_rr"], res["n_lr"])] == [10] * 5
    assert res["n_ll"] == [0, 1, 3, 6, 10] and res["n_rr"] == [6, 3, 1, 0, 0]
    assert len(set(res["zns_r2"])) == 1 and res["zns_r2"][0] == sum(Q5.values()) / 10e6


def test_two_sites_at_one_position_and_half_window_0():
    sites = ["s1", "s2", "s3", "s4"]
    where = [("c", 100), ("c", 200), ("c", 200), ("c", 300)]
    text = _row(sites[0], sites[1], "100", "0.300000") + "\n" + _row(sites[1], sites[2], "0", "0.700000") + "\n"
    res = scan_ref.scan(text, sites, 0, positions=where)
    # the two sites share a window; the row between them is across site 1 (its right flank holds site 2) and left of site 2
    assert res["win_first"] == [0, 1, 1, 3] and res["win_last"] == [0, 2, 2, 3]
    assert res["n_ll"] == [0, 0, 1, 0] and res["n_rr"] == [0, 0, 0, 0] and res["n_lr"] == [0, 1, 0, 0]
    assert res["sum_lr_r2"] == [0, 700000, 0, 0] and res["sum_ll_r2"] == [0, 0, 700000, 0]
    assert res["zns_r2"] == [None, 0.7, 0.7, None] and res["omega_r2"] == [None] * 4
    assert scan_ref.scan(text, sites, 0, positions=where, brute=True) == res
    assert scan_ref.positions_of(["c:200\tx", "chr1:7"]) == [("c", 200), ("chr1", 7)]


def test_two_chromosomes():
    sites = ["A:100", "A:200", "B:100", "B:200"]
    rows = [_row(sites[0], sites[1], "100", "0.250000"), _row(sites[0], sites[2], "inf", "0.990000"),
            _row(sites[1], sites[2], "inf", "0.990000"), _row(sites[2], sites[3], "100", "0.500000")]
    res = scan_ref.scan("\n".join(rows) + "\n", sites, 1000)
    assert res["win_first"] == [0, 0, 2, 2] and res["win_last"] == [1, 1, 3, 3]
    assert res["n_lr"] == [1, 0, 1, 0] and res["n_ll"] == [0, 1, 0, 1] and res["n_rr"] == [0] * 4
    assert res["sum_lr_r2"] == [250000, 0, 500000, 0] and res["sum_ll_r2"] == [0, 250000, 0, 500000]


def test_a_nan_row_drops_out_of_every_statistic_and_the_filters():
    sites = ["c:1", "c:2", "c:3"]
    rows = [_row(sites[0], sites[1], "1", "0.200000", d="-0.100000"), _row(sites[0], sites[2], "2", "nan", d="0.300000"),
            _row(sites[1], sites[2], "1", "0.400000", d="-inf")]
    text = "\n".join(rows) + "\n"
    both = scan_ref.scan(text, sites, 5, ld=("D", "r2"))
    assert [both[f"n_{c}"][1] for c in scan_ref.CLASSES] == [1, 0, 0]  # (only the first row is finite in D and r2)
    assert both["sum_ll_D"][1] == 100000 and both["sum_ll_r2"][1] == 200000  # (|D|)
    r2 = scan_ref.scan(text, sites, 5, ld=("r2",))
    assert [r2[f"n_{c}"][1] for c in scan_ref.CLASSES] == [1, 0, 1]  # (0,1) left of site 1, (1,2) across it
    d = scan_ref.scan(text, sites, 5, ld=("D",))
    assert [d[f"n_{c}"][1] for c in scan_ref.CLASSES] == [1, 0, 1] and d["sum_lr_D"][1] == 300000  # (0,2) across site 1
    near = scan_ref.scan(text, sites, 5, ld=("D",), max_kb_dist=0.001)
    assert [near[f"n_{c}"][1] for c in scan_ref.CLASSES] == [1, 0, 0]  # (dist 2 is beyond 1 bp)


def test_every_omega_na_case_and_the_file():
    sites = ["c:10", "c:20", "c:30", "z:5"]
    rows = [_row(sites[0], sites[1], "10", "0.000000"), _row(sites[0], sites[2], "20", "0.000000"),
            _row(sites[1], sites[2], "10", "0.125000")]
    text = "\n".join(rows) + "\n"
    res = scan_ref.scan(text, sites, 100)
    # site 0: (1,2) right of it, two rows across that print 0 -- S_LR == 0 with rows present; site 1: (0,1) left, two rows
    # across; site 2: nothing across; site 3: no row at all
    assert res["n_ll"] == [0, 1, 3, 0] and res["n_rr"] == [1, 0, 0, 0] and res["n_lr"] == [2, 2, 0, 0]
    assert res["sum_lr_r2"] == [0, 125000, 0, 0]
    assert res["omega_r2"] == [None, 0.0, None, None] and res["zns_r2"][3] is None
    # a narrower window: site 0 no longer sees (1,2), nothing is inside a flank
    res = scan_ref.scan(text, sites, 10)
    assert res["win_last"][:3] == [1, 2, 2]
    assert (res["n_ll"][0], res["n_rr"][0], res["n_lr"][0]) == (0, 0, 1) and res["omega_r2"][0] is None and res["zns_r2"][0] == 0.0
    two = scan_ref.scan("\n".join(rows[:2]) + "\n", sites, 100)
    assert (two["n_ll"][1], two["n_lr"][1], two["sum_lr_r2"][1]) == (1, 1, 0) and two["omega_r2"][1] is None and two["zns_r2"][1] == 0.0
    want = ("site\twin_sites\tleft_sites\tright_sites\tn_ll\tn_rr\tn_lr\tsum_ll_r2\tsum_rr_r2\tsum_lr_r2\tzns_r2\tomega_r2\n"
            "c:10\t3\t1\t2\t0\t1\t2\t0.000000\t0.125000\t0.000000\t0.041666666666666664\tNA\n"
            "c:20\t3\t2\t1\t1\t0\t2\t0.000000\t0.000000\t0.125000\t0.041666666666666664\t0\n"
            "c:30\t3\t3\t0\t3\t0\t0\t0.125000\t0.000000\t0.000000\t0.041666666666666664\tNA\n"
            "z:5\t1\t1\t0\t0\t0\t0\t0.000000\t0.000000\t0.000000\tNA\tNA\n")
    assert scan_ref.scan_file(text, sites, 100) == want
    assert scan_ref.scan_file(text, sites, 100, names=["1", "2", "3", "4"]).splitlines()[2].startswith("2\t3\t2\t1\t")
    # without positions every window is its own site and nothing is counted anywhere
    nopos = scan_ref.scan(text, sites, 100, positions=scan_ref.NO_POS)
    assert nopos["win_first"] == nopos["win_last"] == [0, 1, 2, 3] and nopos["n_ll"] == nopos["n_lr"] == [0] * 4


def test_range_decomposition_equals_the_definition_on_random_layouts():
    rng = random.Random(20251020)
    classes_seen, empty_ranges = set(), 0
    for layout in range(300):
        n = rng.randrange(2, 26)
        n_chr = rng.randrange(1, 4)
        positions, pos, chrom = [], 0, 0
        for s in range(n):
            if s and chrom + 1 < n_chr and rng.random() < 0.15:
                chrom, pos = chrom + 1, 0
            pos += rng.choice([0, 0, 1, 3, 10, 50])  # (repeated positions)
            positions.append((f"k{chrom}", pos))
        span = max(p for _, p in positions)
        half = rng.choice([0, 1, 5, 20, span // 2, span, span + 1, 10 * span + 7])
        a, b = scan_ref.windows(positions, n, half)
        for c in range(n):
            assert a[c] <= c <= b[c]
            assert all(positions[s][0] == positions[c][0] and abs(positions[s][1] - positions[c][1]) <= half for s in range(a[c], b[c] + 1))
            for s in (a[c] - 1, b[c] + 1):
                assert not 0 <= s < n or positions[s][0] != positions[c][0] or abs(positions[s][1] - positions[c][1]) > half
        # rows: a random subset of the pairs on one chromosome, whatever their distance
        rows = [(i, j, (rng.randrange(0, 2 ** 38), rng.randrange(0, 3)))
                for i in range(n) for j in range(i + 1, n) if positions[i][0] == positions[j][0] and rng.random() < 0.7]
        fast = scan_ref.scan_rows(rows, a, b, ["D", "r2"])
        slow = scan_ref.scan_rows(rows, a, b, ["D", "r2"], brute=True)
        assert fast == slow, (layout, positions, half)
        for i, j, _ in rows:
            for k, (x, y) in enumerate(scan_ref.ranges_of(i, j, a, b)):
                empty_ranges += x > y
                assert [c for c in range(n) if a[c] <= i and j <= b[c] and scan_ref.class_of(i, j, c) == k] == list(range(x, y + 1))
                if x <= y:
                    classes_seen.add(k)
    assert classes_seen == {0, 1, 2} and empty_ranges > 100


def test_micro_and_text_round_trip():
    for t in ("0.000000", "1.000000", "-0.031250", "274877.906943"):
        assert scan_ref.micro_text(scan_ref.micro(t)) == t
    assert scan_ref.micro("nan") is None and scan_ref.micro("-inf") is None and math.isnan(float("nan"))
