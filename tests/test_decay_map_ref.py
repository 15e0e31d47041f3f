"""tests/decay_map_ref.py -- the yardstick of ngsld_decay_map -- on a hand-written table with the answer written out: a midpoint
exactly on a window's edge and one below it, two sites at one position, a pair whose window holds neither of its sites, a
chromosome of one site, a row that a NaN takes out of every statistic, and the groups adding up to decay_ref's pooled bins."""
from fractions import Fraction as Fr

import decay_map_ref
import decay_ref

HEAD = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"
# W = 100 (2 W = 200), B = 50; chromosome A has sites at 10, 89, 90, 110, 110 (two sites), 290, 500; B one site; C two
ROWS = [
    # site1   site2   dist    D            r2            p1 + p2 -> w   bin
    ("A:10", "A:89", "79", "-0.010000", "0.100000"),     # 99 -> 0        50
    ("A:10", "A:90", "80", "-0.010000", "0.300000"),     # 100 -> 0       50
    ("A:89", "A:110", "21", "-0.010000", "0.500000"),    # 199 -> 0 (one below 2 W)       0
    ("A:90", "A:110", "20", "-0.010000", "0.700000"),    # 200 -> 1 (exactly 2 W)         0
    ("A:110", "A:110", "0", "-0.010000", "0.900000"),    # two sites at one position: dist 0 is in no bin
    ("A:10", "A:290", "280", "-0.010000", "0.020000"),   # 300 -> 1: sites in windows 0 and 2      250
    ("A:10", "A:500", "490", "-0.010000", "0.010000"),   # 510 -> 2: sites in windows 0 and 5      450
    ("A:90", "A:110", "20", "-0.010000", "0.200000"),    # (the second site at 110) 200 -> 1       0
    ("A:110", "A:290", "180", "-0.010000", "0.050000"),  # 400 -> 2 (exactly 2 W * 2)              150
    ("A:290", "A:500", "210", "0.200000", "-nan"),       # 790 -> 3: the NaN drops the row from D too; group (A, 3) has no bin
    ("A:500", "B:50", "inf", "-0.010000", "0.400000"),   # across chromosomes: never counted
    ("B:50", "C:1000", "inf", "-0.010000", "0.400000"),  # ... so the one-site chromosome B has no group
    ("C:1000", "C:1100", "100", "-0.010000", "0.600000"),  # 2100 -> 10; dist 100 is in (50, 100]          50
]
TABLE = HEAD + "".join(f"{a}\t{b}\t{d}\t0.000000\t{D}\t0.000000\t{r2}\n" for a, b, d, D, r2 in ROWS)
D = Fr(-1, 100)


def _bins(*entries):
    return [(float(dist), n, {"D": D, "r2": r2}) for dist, n, r2 in entries]


def test_windows_by_hand():
    got = decay_map_ref.decay_map(TABLE, window=100, ld=("r2", "D"), bin_size=50)
    assert got == [
        ("A", 0, _bins((0, 1, Fr(1, 2)), (50, 2, Fr(1, 5)))),
        ("A", 100, _bins((0, 2, Fr(9, 20)), (250, 1, Fr(1, 50)))),
        ("A", 200, _bins((150, 1, Fr(1, 20)), (450, 1, Fr(1, 100)))),
        ("C", 1000, _bins((50, 1, Fr(3, 5)))),
    ]


def test_chromosomes_by_hand():
    got = decay_map_ref.decay_map(TABLE, ld=("r2", "D"), bin_size=50)
    assert got == [
        ("A", 0, _bins((0, 3, Fr(7, 15)), (50, 2, Fr(1, 5)), (150, 1, Fr(1, 20)), (250, 1, Fr(1, 50)), (450, 1, Fr(1, 100)))),
        ("C", 0, _bins((50, 1, Fr(3, 5)))),
    ]


def test_a_window_beyond_every_position_is_the_chromosome():
    by_chr = decay_map_ref.decay_map(TABLE, ld=("r2", "D"), bin_size=50)
    assert decay_map_ref.decay_map(TABLE, window=10 ** 6, ld=("r2", "D"), bin_size=50) == by_chr


def test_strict_limit_and_bin_size_reach_every_group():
    got = decay_map_ref.decay_map(TABLE, window=100, bin_size=100, max_kb_dist=0.28)  # (dist 280 is out: strict)
    assert got == [
        ("A", 0, [(0.0, 3, {"r2": Fr(3, 10)})]),
        ("A", 100, [(0.0, 2, {"r2": Fr(9, 20)})]),
        ("A", 200, [(100.0, 1, {"r2": Fr(1, 20)})]),
        ("C", 1000, [(0.0, 1, {"r2": Fr(3, 5)})]),
    ]


def test_groups_add_up_to_the_pooled_bins():
    within = HEAD + "".join(ln + "\n" for ln in TABLE.splitlines()[1:] if ln.split("\t")[0].split(":")[0] == ln.split("\t")[1].split(":")[0])
    for table in (within, TABLE):  # (decay_ref drops the rows across chromosomes itself: their dist is not finite)
        for window in (0, 100, 37):
            pooled = decay_ref.decay_bins(table, ld=("r2", "D"), bin_size=50)
            n, sums = {}, {}
            for _, _, bins in decay_map_ref.decay_map(table, window=window, ld=("r2", "D"), bin_size=50):
                for dist, cnt, mean in bins:
                    n[dist] = n.get(dist, 0) + cnt
                    for f, m in mean.items():
                        sums[dist, f] = sums.get((dist, f), 0) + m * cnt
            assert sorted(n) == [b[0] for b in pooled]
            for dist, cnt, mean in pooled:
                assert n[dist] == cnt
                assert all(sums[dist, f] == m * cnt for f, m in mean.items())
