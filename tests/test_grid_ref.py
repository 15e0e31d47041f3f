"""tests/grid_ref.py -- the yardstick of ngsld_grid -- held to TSVs small enough to work by hand (GRID.md has the rule)."""
import math

import grid_ref
import site_ref

HEAD7 = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"


def _row(a, b, dist, r2e="0.100000", D="0.010000", Dp="0.500000", r2="0.250000", maf=None):
    cells = [a, b, dist, r2e, D, Dp, r2]
    if maf:
        cells += ["10", maf[0], maf[1]] + ["0.000000"] * 9
    return "\t".join(cells) + "\n"


def _cells(got, *names):
    return [tuple(got[k][i] for k in ("chr", "bin1", "bin2", *names)) for i in range(len(got["n"]))]


def test_a_position_on_the_break_opens_the_next_bin():
    sites = ["c:5", "c:99", "c:100", "c:199", "c:200"]
    text = HEAD7 + _row("c:5", "c:99", "94") + _row("c:5", "c:100", "95") + _row("c:99", "c:100", "1") + \
        _row("c:100", "c:199", "99") + _row("c:199", "c:200", "1")
    got = grid_ref.grid(text, sites, 100)
    # c:99 = k * B - 1 stays in bin 0, c:100 = k * B is bin 1; bins are reported at their lower break b * B
    assert _cells(got, "n") == [("c", 0, 0, 1), ("c", 0, 100, 2), ("c", 100, 100, 1), ("c", 100, 200, 1)]
    assert got["sum_r2"] == [250000, 500000, 250000, 250000] and got["mean_r2"] == [0.25] * 4
    # a bin size of 1: every position its own bin; 2^31 - 1: one cell
    assert _cells(grid_ref.grid(text, sites, 1), "n")[0] == ("c", 5, 99, 1)
    assert _cells(grid_ref.grid(text, sites, 2 ** 31 - 1), "n") == [("c", 0, 0, 5)]


def test_a_pair_counts_once_in_one_cell_and_empty_cells_are_absent():
    sites = ["c:10", "c:20", "c:310", "c:320"]
    text = HEAD7 + _row("c:10", "c:20", "10", r2="0.250000") + _row("c:10", "c:310", "300", r2="0.750000") + \
        _row("c:20", "c:320", "300", r2="0.500000")
    got = grid_ref.grid(text, sites, 100)
    # (bin 0, bin 0) holds the pair inside one window; (0, 300) both long pairs; nothing in (0, 100), (0, 200), (300, 300): absent
    assert _cells(got, "n", "sum_r2", "max_r2", "linked_r2", "mean_r2") == [
        ("c", 0, 0, 1, 250000, 250000, 0, 0.25), ("c", 0, 300, 2, 1250000, 750000, 2, 0.625)]
    assert sum(got["n"]) == 3  # (once, not at both ends)
    assert grid_ref.grid_file(text, sites, 100) == ("chr\tbin1\tbin2\tn\tsum_r2\tmean_r2\tmax_r2\tlinked_r2\n"
                                                    "c\t0\t0\t1\t0.250000\t0.25\t0.250000\t0\n"
                                                    "c\t0\t300\t2\t1.250000\t0.625\t0.750000\t2\n")


def test_two_sites_at_one_position_share_their_bin():
    sites = ["c:250", "c:250", "c:260"]  # (the TSV prints the same label for both)
    text = HEAD7 + _row("c:250", "c:250", "0", r2="0.100000") + _row("c:250", "c:260", "10", r2="0.300000") + \
        _row("c:250", "c:260", "10", r2="0.500000")
    got = grid_ref.grid(text, sites, 100)
    assert _cells(got, "n", "sum_r2", "max_r2") == [("c", 200, 200, 3, 900000, 500000)]
    assert _cells(grid_ref.grid(text, sites, 10), "n") == [("c", 250, 250, 1), ("c", 250, 260, 2)]


def test_a_nan_statistic_drops_the_row_for_every_statistic():
    sites = ["c:1", "c:2", "c:3", "c:4"]
    text = HEAD7 + _row("c:1", "c:2", "1", Dp="-nan") + _row("c:2", "c:3", "1", D="inf") + _row("c:3", "c:4", "1")
    both = grid_ref.grid(text, sites, 100, ld=("r2", "Dp", "D"))
    assert both["n"] == [1] and both["sum_r2"] == [250000] and both["sum_Dp"] == [500000]
    assert grid_ref.grid(text, sites, 100, ld=("r2",))["n"] == [3]  # (r2 alone is finite in every row)


def test_a_value_exactly_linked_min_is_linked():
    sites = ["c:1", "c:2", "c:3", "c:4"]
    text = HEAD7 + _row("c:1", "c:2", "1", r2="0.500000") + _row("c:1", "c:3", "2", r2="0.499999") + _row("c:1", "c:4", "3", r2="0.100000")
    assert grid_ref.grid(text, sites, 100)["linked_r2"] == [1]
    # 0.1 is not a double: the printed 0.100000 reads back as the same double as the limit 0.1 and is linked
    assert grid_ref.grid(text, sites, 100, linked_min=0.1)["linked_r2"] == [3]
    assert grid_ref.grid(text, sites, 100, linked_min=math.nextafter(0.1, 1.0))["linked_r2"] == [2]


def test_dist_on_the_limit_is_in_and_beyond_it_out():
    sites = ["c:1", "c:1001", "c:1002"]
    text = HEAD7 + _row("c:1", "c:1001", "1000") + _row("c:1", "c:1002", "1001")
    assert _cells(grid_ref.grid(text, sites, 500, max_kb_dist=1.0), "n") == [("c", 0, 1000, 1)]
    assert _cells(grid_ref.grid(text, sites, 500, max_kb_dist=1.5), "n") == [("c", 0, 1000, 2)]
    assert grid_ref.grid(text, sites, 500, max_kb_dist=1.001)["n"] == [1]  # (1.001 * 1000 is 1000.9999999999999)
    assert grid_ref.grid(text, sites, 500, max_kb_dist=0.0)["n"] == []


def test_two_chromosomes_in_file_order_and_no_cell_across_them():
    sites = ["z:150", "z:160", "a:10", "a:150"]
    text = HEAD7 + _row("z:150", "z:160", "10") + _row("z:160", "a:10", "inf", r2="0.900000") + _row("a:10", "a:150", "140", r2="0.600000")
    got = grid_ref.grid(text, sites, 100)
    # z before a: the order of the file, not of the names; the row across the chromosomes (dist inf) is in no cell
    assert _cells(got, "n", "max_r2") == [("z", 100, 100, 1, 250000), ("a", 0, 100, 1, 600000)]


def test_signed_against_absolute_d():
    sites = ["c:1", "c:2", "c:3"]
    text = HEAD7 + _row("c:1", "c:2", "1", D="-0.200000") + _row("c:1", "c:3", "2", D="0.050000")
    a = grid_ref.grid(text, sites, 100, ld=("D",), linked_min=0.1)
    assert (a["sum_D"], a["max_D"], a["linked_D"]) == ([250000], [200000], [1])
    s = grid_ref.grid(text, sites, 100, ld=("D",), linked_min=0.1, abs_value=False)
    assert (s["sum_D"], s["max_D"], s["linked_D"], s["mean_D"]) == ([-150000], [50000], [0], [-0.075])
    assert grid_ref.grid_file(text, sites, 100, ld=("D",), abs_value=False).splitlines()[1] == \
        "c\t0\t0\t2\t-0.150000\t-0.074999999999999997\t0.050000\t0"


def test_the_maf_filter_reads_the_printed_maf():
    sites = ["c:1", "c:2", "c:3"]
    text = "\t".join(site_ref.COLUMNS) + "\n" + _row("c:1", "c:2", "1", maf=("0.100000", "0.300000")) + \
        _row("c:1", "c:3", "2", maf=("0.100000", "0.099999")) + _row("c:2", "c:3", "1", maf=("0.300000", "-nan"))
    assert grid_ref.grid(text, sites, 100, min_maf=0.1)["n"] == [1]
    assert grid_ref.grid(text, sites, 100)["n"] == [2]  # (a NaN maf never passes, whatever the limit)


def test_the_mean_is_rounded_once():
    sites = ["c:1", "c:2", "c:3", "c:4"]
    rows = "".join(_row("c:1", f"c:{k}", "1", r2=t) for k, t in ((2, "0.100000"), (3, "0.100000"), (4, "0.100001")))
    got = grid_ref.grid(HEAD7 + rows, sites, 100)
    assert got["sum_r2"] == [300001] and got["mean_r2"] == [300001 / 3000000]  # (int / int: the nearest double)
