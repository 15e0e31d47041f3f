"""tests/cross_ref.py -- the plain-Python rule of CROSS.md that tests/test_gpu_cross.py holds the device to -- against a table
worked by hand: three chromosomes (one of a single site), rows across them with dist inf, a NaN row.  No GPU."""
from fractions import Fraction

import cross_ref

SITES = ["a:100", "a:250", "b:50", "c:10", "c:2100"]
# site1 site2 dist r2_ExpG D Dp r2
TABLE = "\n".join("\t".join(r.split()) for r in """
a:100 a:250 150 0.100000 0.050000 0.500000 0.250000
a:100 b:50 inf 0.010000 -0.020000 -0.300000 0.040000
a:100 c:10 inf 0.020000 0.010000 0.100000 0.600000
a:100 c:2100 inf nan nan nan nan
a:250 b:50 inf 0.030000 0.030000 0.700000 0.090000
a:250 c:10 inf 0.040000 -0.010000 -0.200000 0.500000
a:250 c:2100 inf 0.050000 0.020000 0.400000 0.010000
b:50 c:10 inf 0.060000 0.040000 0.900000 0.810000
b:50 c:2100 inf 0.070000 -0.050000 -1.000000 1.000000
c:10 c:2100 2090 0.080000 0.060000 0.600000 0.360000
""".strip().splitlines()) + "\n"


def _keys(res):
    return list(zip(res["chr1"], res["bin1"], res["chr2"], res["bin2"]))


def test_one_bin_per_chromosome():
    res = cross_ref.cross(TABLE, SITES)
    assert _keys(res) == [("a", 0, "a", 0), ("a", 0, "b", 0), ("a", 0, "c", 0), ("b", 0, "c", 0), ("c", 0, "c", 0)]
    assert res["n"] == [1, 2, 3, 2, 1]  # (the NaN row of a - c is in no cell; the one-site chromosome has no cell of its own)
    assert res["sum_r2"] == [250000, 130000, 1110000, 1810000, 360000]
    assert res["max_r2"] == [250000, 90000, 600000, 1000000, 360000]
    assert res["linked_r2"] == [0, 0, 2, 2, 0]  # (0.5 itself is linked)
    assert res["mean_r2"] == [0.25, 0.065, 0.37, 0.905, 0.36]
    assert res["mean_r2"][2] == float(Fraction(1110000, 3 * 10 ** 6))
    assert cross_ref.cross(TABLE, SITES, 10 ** 9) == res


def test_windows_are_numbered_over_the_chromosomes():
    res = cross_ref.cross(TABLE, SITES, 1000)
    assert cross_ref.gbins(SITES, 1000) == {"a:100": (0, "a", 0), "a:250": (0, "a", 0), "b:50": (1, "b", 0), "c:10": (2, "c", 0),
                                            "c:2100": (4, "c", 2)}
    assert _keys(res) == [("a", 0, "a", 0), ("a", 0, "b", 0), ("a", 0, "c", 0), ("a", 0, "c", 2000), ("b", 0, "c", 0),
                          ("b", 0, "c", 2000), ("c", 0, "c", 2000)]
    assert res["n"] == [1, 2, 2, 1, 1, 1, 1]
    assert res["sum_r2"] == [250000, 130000, 1100000, 10000, 810000, 1000000, 360000]


def test_signed_values_and_several_statistics():
    res = cross_ref.cross(TABLE, SITES, ld=("r2", "Dp", "D"), abs_value=False, linked_min=0.04)
    assert [k for k in res if k.startswith("sum_")] == ["sum_D", "sum_Dp", "sum_r2"]  # (TSV column order)
    assert res["sum_Dp"] == [500000, 400000, 300000, -100000, 600000]
    assert res["max_Dp"] == [500000, 700000, 400000, 900000, 600000]
    assert res["sum_D"] == [50000, 10000, 20000, -10000, 60000] and res["linked_D"] == [1, 0, 0, 1, 1]
    both = cross_ref.cross(TABLE, SITES, ld=("Dp",))
    assert both["sum_Dp"] == [500000, 1000000, 700000, 1900000, 600000]


def test_only_across_chromosomes_and_the_floor_inside_one():
    res = cross_ref.cross(TABLE, SITES, within=False)
    assert _keys(res) == [("a", 0, "b", 0), ("a", 0, "c", 0), ("b", 0, "c", 0)] and res["n"] == [2, 3, 2]
    res = cross_ref.cross(TABLE, SITES, min_kb_dist=1.0)  # (150 bp is below it, 2,090 bp is not; rows across are not asked)
    assert _keys(res) == [("a", 0, "b", 0), ("a", 0, "c", 0), ("b", 0, "c", 0), ("c", 0, "c", 0)]
    assert cross_ref.cross(TABLE, SITES, min_kb_dist=2.09)["n"] == [2, 3, 2, 1]
    assert cross_ref.cross(TABLE, SITES, min_kb_dist=2.091)["n"] == [2, 3, 2]


def test_the_maf_filter_reads_the_extended_columns():
    head = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\tsample_size\tmaf1\tmaf2\n"
    rows = "".join(f"{ln}\t8\t{m1}\t{m2}\n" for ln, (m1, m2) in zip(TABLE.splitlines(), [
        ("0.100000", "0.200000"), ("0.100000", "0.050000"), ("0.100000", "0.100000"), ("0.100000", "0.300000"),
        ("0.200000", "0.050000"), ("0.200000", "0.100000"), ("0.200000", "0.300000"), ("0.050000", "0.100000"),
        ("0.050000", "nan"), ("0.100000", "0.300000")]))
    res = cross_ref.cross(head + rows, SITES, min_maf=0.1)
    assert _keys(res) == [("a", 0, "a", 0), ("a", 0, "c", 0), ("c", 0, "c", 0)] and res["n"] == [1, 3, 1]


def test_the_file():
    assert cross_ref.cross_file(TABLE, SITES, 1000, ld=("r2",)).splitlines()[:4] == [
        "chr1\tbin1\tchr2\tbin2\tn\tsum_r2\tmean_r2\tmax_r2\tlinked_r2",
        "a\t0\ta\t0\t1\t0.250000\t0.25\t0.250000\t0",
        "a\t0\tb\t0\t2\t0.130000\t0.065000000000000002\t0.090000\t0",
        "a\t0\tc\t0\t2\t1.100000\t0.55000000000000004\t0.600000\t2"]
