"""tests/blocks_ref.py -- the restatement of scripts/LD_blocks.sh that ngsld_blocks is held to -- against hand-worked TSVs, no
GPU: which rows are in the region, which sites make the matrix and in what order, where each cell lands and its text."""
import pytest

import blocks_ref

HEAD = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"


def row(a, b, dist, r2e, d, dp, r2, extra=""):
    return f"{a}\t{b}\t{dist}\t{r2e}\t{d}\t{dp}\t{r2}{extra}\n"


def test_inside_a_chromosome_bounds_inclusive_and_outside_pairs_dropped():
    text = HEAD + "".join([
        row("c1:5", "c1:10", 5, "0.1", "0.01", "0.2", "0.3"),       # 5 < START: out
        row("c1:10", "c1:20", 10, "0.100000", "-0.010000", "0.250000", "0.500000"),
        row("c1:10", "c1:30", 20, "0.2", "0.02", "0.3", "0.4"),
        row("c1:10", "c2:15", "inf", "0.1", "0.1", "0.1", "0.1"),    # other chromosome: out
        row("c1:20", "c1:30", 10, "0.3", "0.03", "0.35", "0.45"),
        row("c1:30", "c1:31", 1, "0.9", "0.09", "0.95", "0.99"),     # 31 > END: out
    ])
    sites, files, info = blocks_ref.blocks(text, "c1", 10, 30)
    assert sites == ["c1:10", "c1:20", "c1:30"]
    assert info["pairs_in_region"] == 3 and info["sites"] == 3
    assert files["r2"] == ("\tc1:10\tc1:20\tc1:30\n"
                           "c1:10\tNA\t0.500000\t0.4\n"
                           "c1:20\tNA\tNA\t0.45\n"
                           "c1:30\tNA\tNA\tNA\n")
    assert files["Dp"].split("\n")[1] == "c1:10\tNA\t0.250000\t0.3"
    assert set(files) == {"r2", "Dp"}


def test_file_order_not_position_order_puts_cells_below_the_diagonal():
    """c1 reappears after c2 in the pos file: its later sites come first in position, so pairs (s1 later in the file, s2
    earlier in position) land below the diagonal, as acast(snp1 ~ snp2) puts them."""
    text = "".join([
        row("c1:100", "c1:200", 100, "0.1", "0.1", "0.1", "0.11"),
        row("c1:200", "c2:5", "inf", "0.1", "0.1", "0.1", "0.1"),
        row("c2:5", "c1:50", "inf", "0.1", "0.1", "0.1", "0.1"),
        row("c1:50", "c1:60", 10, "0.2", "0.2", "0.2", "0.22"),
        row("c1:200", "c1:50", "inf", "0.1", "0.1", "0.1", "0.33"),   # (a TSV row across the reappearance)
    ])
    sites, files, info = blocks_ref.blocks(text, "c1", 1, 1000, ld=("r2",))
    assert sites == ["c1:50", "c1:60", "c1:100", "c1:200"]
    lines = files["r2"].split("\n")
    assert lines[0] == "\tc1:50\tc1:60\tc1:100\tc1:200"
    assert lines[1] == "c1:50\tNA\t0.22\tNA\tNA"
    assert lines[3] == "c1:100\tNA\tNA\tNA\t0.11"
    assert lines[4] == "c1:200\t0.33\tNA\tNA\tNA"                 # below the diagonal
    assert info["pairs_in_region"] == 3


def test_sites_only_as_snp2_or_only_as_snp1_are_rows_and_columns():
    text = HEAD + row("c1:1", "c1:3", 2, "0.1", "0.2", "0.3", "0.4") + row("c1:2", "c1:3", 1, "0.5", "0.6", "0.7", "0.8")
    sites, files, _ = blocks_ref.blocks(text, "c1", 1, 3, ld=("D",))
    assert sites == ["c1:1", "c1:2", "c1:3"]                      # c1:1, c1:2 only as snp1, c1:3 only as snp2
    assert files["D"] == "\tc1:1\tc1:2\tc1:3\nc1:1\tNA\tNA\t0.2\nc1:2\tNA\tNA\t0.6\nc1:3\tNA\tNA\tNA\n"


def test_nan_and_negative_zero_cells_keep_their_text():
    text = HEAD + row("c1:1", "c1:2", 1, "-nan", "-0.000000", "nan", "inf") + row("c1:1", "c1:4", 3, "0", "1", "2", "-nan")
    _, files, _ = blocks_ref.blocks(text, "c1", 1, 4, ld=blocks_ref.FIELDS)
    assert files["r2_ExpG"].split("\n")[1] == "c1:1\tNA\t-nan\t0"
    assert files["D"].split("\n")[1] == "c1:1\tNA\t-0.000000\t1"
    assert files["Dp"].split("\n")[1] == "c1:1\tNA\tnan\t2"
    assert files["r2"].split("\n")[1] == "c1:1\tNA\tinf\t-nan"


def test_extended_columns_are_cut():
    text = row("c1:1", "c1:2", 1, "0.1", "0.2", "0.3", "0.4", extra="\t64\t0.1\t0.2\t0.25\t0.25\t0.25\t0.25\t0.5\t0.5\t0.1\t0.0\t3")
    _, files, _ = blocks_ref.blocks(text, "c1", 1, 2, ld=("r2",))
    assert files["r2"] == "\tc1:1\tc1:2\nc1:1\tNA\t0.4\nc1:2\tNA\tNA\n"


def test_chr_is_matched_byte_for_byte():
    text = row("chr1:1", "chr1:2", 1, "0", "0", "0", "0.5") + row("chr10:1", "chr10:2", 1, "0", "0", "0", "0.6")
    sites, files, _ = blocks_ref.blocks(text, "chr1", 1, 2, ld=("r2",))
    assert sites == ["chr1:1", "chr1:2"] and "0.6" not in files["r2"]


def test_no_pair_in_region_gives_the_label_row_only():
    sites, files, info = blocks_ref.blocks(HEAD + row("c1:1", "c1:50", 49, "0", "0", "0", "0"), "c1", 1, 10, ld=("r2",))
    assert sites == [] and files["r2"] == "\n" and info["pairs_in_region"] == 0


def test_null_labels_are_refused():
    with pytest.raises(blocks_ref.Refused) as e:
        blocks_ref.blocks(HEAD + row("(null)", "(null)", "inf", "0", "0", "0", "0"), "c1", 1, 10)
    assert e.value.kind == "invalid"


def test_repeated_position_is_refused():
    text = row("c1:100", "c1:150", 50, "0", "0", "0", "0") + row("c1:0100", "c1:120", 20, "0", "0", "0", "0")
    with pytest.raises(blocks_ref.Refused) as e:
        blocks_ref.blocks(text, "c1", 1, 1000)
    assert e.value.kind == "unsupported" and "share a position" in str(e.value)


@pytest.mark.parametrize("label", ["c1:12a", "c1:", "c1:-5", "c1:1e3", "c1"])
def test_bad_position_of_a_candidate_is_refused(label):
    with pytest.raises(blocks_ref.Refused) as e:
        blocks_ref.blocks(row("c1:1", label, 1, "0", "0", "0", "0"), "c1", 1, 10)
    assert e.value.kind == "unsupported" and label in str(e.value)


def test_bad_position_of_another_chromosome_is_no_concern():
    text = row("c1:1", "c1:2", 1, "0", "0", "0", "0.5") + row("c2:x", "c2:y", 1, "0", "0", "0", "0")
    sites, _, _ = blocks_ref.blocks(text, "c1", 1, 2, ld=("r2",))
    assert sites == ["c1:1", "c1:2"]
