"""tests/site_ref.py -- the yardstick of ngsld_site_ld -- held to TSVs small enough to work by hand (SITES.md has the rule)."""
import math

import site_ref

HEAD7 = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"
SITES = ["c:1", "c:2", "c:3", "c:4", "d:1"]


def _row(a, b, dist, r2e="0.100000", D="0.010000", Dp="0.500000", r2="0.250000", maf=None):
    cells = [a, b, dist, r2e, D, Dp, r2]
    if maf:
        cells += ["10", maf[0], maf[1]] + ["0.000000"] * 9
    return "\t".join(cells) + "\n"


def test_micro_reads_the_text_with_integers():
    assert site_ref.micro("0.123456") == 123456 and site_ref.micro("-12.000001") == -12000001
    assert site_ref.micro("-0.000000") == 0 and site_ref.micro("274877.906943") == 274877906943
    assert all(site_ref.micro(t) is None for t in ("nan", "-nan", "inf", "-inf"))
    assert site_ref.micro_text(-1) == "-0.000001" and site_ref.micro_text(0) == "0.000000" and site_ref.micro_text(12345678) == "12.345678"


def test_a_pair_counts_at_both_ends():
    text = HEAD7 + _row("c:1", "c:2", "10", r2="0.250000") + _row("c:1", "c:3", "20", r2="0.750000")
    got = site_ref.site_ld(text, SITES)
    assert got["n"] == [2, 1, 1, 0, 0]
    assert got["sum_r2"] == [1000000, 250000, 750000, 0, 0]
    assert got["max_r2"] == [750000, 250000, 750000, None, None]
    assert got["linked_r2"] == [1, 0, 1, 0, 0]
    assert got["mean_r2"] == [0.5, 0.25, 0.75, None, None]


def test_dist_on_the_limit_is_in_and_beyond_it_out():
    text = HEAD7 + _row("c:1", "c:2", "1000") + _row("c:1", "c:3", "1001")
    assert site_ref.site_ld(text, SITES, max_kb_dist=1.0)["n"] == [1, 1, 0, 0, 0]
    assert site_ref.site_ld(text, SITES, max_kb_dist=1.5)["n"] == [2, 1, 1, 0, 0]
    # the limit is the double max_kb_dist * 1000, as in the library: 1.001 * 1000 is 1000.9999999999999
    assert site_ref.site_ld(text, SITES, max_kb_dist=1.001)["n"] == [1, 1, 0, 0, 0]
    assert site_ref.site_ld(text, SITES, max_kb_dist=0.0)["n"] == [0, 0, 0, 0, 0]


def test_a_nan_statistic_drops_the_row_for_every_statistic():
    text = HEAD7 + _row("c:1", "c:2", "10", Dp="-nan") + _row("c:2", "c:3", "10", D="inf") + _row("c:3", "c:4", "10")
    both = site_ref.site_ld(text, SITES, ld=("r2", "Dp", "D"))
    assert both["n"] == [0, 0, 1, 1, 0] and both["sum_r2"] == [0, 0, 250000, 250000, 0]
    assert site_ref.site_ld(text, SITES, ld=("r2",))["n"] == [1, 2, 2, 1, 0]  # (r2 alone is finite in every row)


def test_inf_dist_never_counts():
    text = HEAD7 + _row("c:4", "d:1", "inf", r2="0.900000") + _row("c:3", "c:4", "5")
    got = site_ref.site_ld(text, SITES)
    assert got["n"] == [0, 0, 1, 1, 0] and got["max_r2"][4] is None and got["mean_r2"][4] is None


def test_minus_zero_is_zero():
    text = HEAD7 + _row("c:1", "c:2", "10", D="-0.000000")
    for abs_value in (True, False):
        got = site_ref.site_ld(text, SITES, ld=("D",), abs_value=abs_value, linked_min=0.0)
        assert got["sum_D"][:2] == [0, 0] and got["max_D"][:2] == [0, 0] and got["linked_D"][:2] == [1, 1]
        assert got["mean_D"][:2] == [0.0, 0.0]
    assert site_ref.site_file(text, SITES[:2], ld=("D",)) == "site\tn\tsum_D\tmean_D\tmax_D\tlinked_D\nc:1\t1\t0.000000\t0\t0.000000\t0\n" \
                                                             "c:2\t1\t0.000000\t0\t0.000000\t0\n"


def test_a_value_exactly_linked_min_is_linked():
    text = HEAD7 + _row("c:1", "c:2", "10", r2="0.500000") + _row("c:1", "c:3", "10", r2="0.499999") + _row("c:1", "c:4", "10", r2="0.100000")
    assert site_ref.site_ld(text, SITES)["linked_r2"] == [1, 1, 0, 0, 0]
    # 0.1 is not a double: the printed 0.100000 reads back as the same double as the limit 0.1 and is linked
    assert site_ref.site_ld(text, SITES, linked_min=0.1)["linked_r2"] == [3, 1, 1, 1, 0]
    assert site_ref.site_ld(text, SITES, linked_min=math.nextafter(0.1, 1.0))["linked_r2"] == [2, 1, 1, 0, 0]


def test_a_site_without_counted_rows_is_na():
    text = HEAD7 + _row("c:1", "c:2", "10")
    assert site_ref.site_file(text, SITES[:3]) == ("site\tn\tsum_r2\tmean_r2\tmax_r2\tlinked_r2\n"
                                                   "c:1\t1\t0.250000\t0.25\t0.250000\t0\n"
                                                   "c:2\t1\t0.250000\t0.25\t0.250000\t0\n"
                                                   "c:3\t0\t0.000000\tNA\tNA\t0\n")
    assert site_ref.site_file(text, SITES[:3], names=["1", "2", "3"]).splitlines()[3] == "3\t0\t0.000000\tNA\tNA\t0"


def test_signed_against_absolute_d():
    text = HEAD7 + _row("c:1", "c:2", "10", D="-0.200000") + _row("c:1", "c:3", "10", D="0.050000")
    a = site_ref.site_ld(text, SITES, ld=("D",), linked_min=0.1)
    assert a["sum_D"][:3] == [250000, 200000, 50000] and a["max_D"][:3] == [200000, 200000, 50000] and a["linked_D"][:3] == [1, 1, 0]
    s = site_ref.site_ld(text, SITES, ld=("D",), linked_min=0.1, abs_value=False)
    assert s["sum_D"][:3] == [-150000, -200000, 50000] and s["max_D"][:3] == [50000, -200000, 50000] and s["linked_D"][:3] == [0, 0, 0]
    assert s["mean_D"][:3] == [-0.075, -0.2, 0.05]
    assert site_ref.site_file(text, SITES, ld=("D",), abs_value=False).splitlines()[2] == "c:2\t1\t-0.200000\t-0.20000000000000001\t-0.200000\t0"


def test_the_maf_filter_reads_the_printed_maf():
    text = "\t".join(site_ref.COLUMNS) + "\n" + _row("c:1", "c:2", "10", maf=("0.100000", "0.300000")) + \
        _row("c:1", "c:3", "10", maf=("0.100000", "0.099999")) + _row("c:2", "c:3", "10", maf=("0.300000", "-nan"))
    assert site_ref.site_ld(text, SITES, min_maf=0.1)["n"] == [1, 1, 0, 0, 0]
    assert site_ref.site_ld(text, SITES)["n"] == [2, 1, 1, 0, 0]  # (a NaN maf never passes, whatever the limit)


def test_the_mean_is_rounded_once():
    rows = "".join(_row("c:1", f"c:{k}", "10", r2=t) for k, t in ((2, "0.100000"), (3, "0.100000"), (4, "0.100001")))
    got = site_ref.site_ld(HEAD7 + rows, SITES)
    assert got["sum_r2"][0] == 300001 and got["mean_r2"][0] == 300001 / 3000000  # (int / int: the nearest double)
