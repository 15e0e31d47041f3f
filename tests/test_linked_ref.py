"""tests/linked_ref.py -- the rule of LINKED.md in plain Python -- held to hand-written tables, no GPU: a value exactly on the
floor, "-0.000000" against a signed floor of 0, nan and inf rows, a row across chromosomes with and without a finite limit, a
NaN maf, labels with an extra column, a table without the extended columns."""
import math

import pytest

import linked_ref

HEAD = ("site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\tsample_size\tmaf1\tmaf2\thap00\thap01\thap10\thap11\thap_maf1\thap_maf2\tchi2\t"
        "loglike\tnIter\n")
TAIL = "0.250000\t0.250000\t0.250000\t0.250000\t0.500000\t0.500000\t0.000000\t0.000000\t3"


def row(a, b, dist, e, d, dp, r2, maf1="0.200000", maf2="0.300000"):
    return f"{a}\t{b}\t{dist}\t{e}\t{d}\t{dp}\t{r2}\t8\t{maf1}\t{maf2}\t{TAIL}"


def names(lines):
    return [tuple(ln.split("\t")[:2]) for ln in lines]


def test_the_floor_itself_passes_and_order_is_the_tables():
    t = HEAD + "\n".join([
        row("c:1", "c:2", 1, "0.100000", "0.010000", "0.300000", "0.500000"),   # on the floor
        row("c:1", "c:3", 2, "0.900000", "0.200000", "1.000000", "0.499999"),   # one unit below
        row("c:2", "c:3", 1, "0.100000", "-0.200000", "-1.000000", "0.500001"),
        row("c:1", "c:4", 3, "0.100000", "0.010000", "0.300000", "1.000000"),
    ]) + "\n"
    got = linked_ref.linked_lines(t)
    assert names(got) == [("c:1", "c:2"), ("c:2", "c:3"), ("c:1", "c:4")]
    assert got[0] == t.splitlines()[1]  # (the line, unchanged)
    assert names(linked_ref.linked_lines(t, min_weight=0.500001)) == [("c:2", "c:3"), ("c:1", "c:4")]
    # the other columns: r2_ExpG, D (absolute and signed), D'
    assert names(linked_ref.linked_lines(t, field=4)) == [("c:1", "c:3")]
    assert names(linked_ref.linked_lines(t, field=5, min_weight=0.2)) == [("c:1", "c:3"), ("c:2", "c:3")]
    assert names(linked_ref.linked_lines(t, field=5, min_weight=0.2, abs_value=False)) == [("c:1", "c:3")]
    assert names(linked_ref.linked_lines(t, field=6, min_weight=-1.0, abs_value=False)) == names(t.splitlines()[1:])
    assert names(linked_ref.linked_lines(t, field=6, min_weight=-0.999999, abs_value=False)) == [("c:1", "c:2"), ("c:1", "c:3"), ("c:1", "c:4")]
    assert linked_ref.linked(t) == "".join(ln + "\n" for ln in got)
    assert linked_ref.linked(t, header=True) == HEAD + "".join(ln + "\n" for ln in got)
    with pytest.raises(ValueError):
        linked_ref.linked_lines(t, field=3)


def test_minus_zero_nan_and_inf_rows():
    t = HEAD + "\n".join([
        row("c:1", "c:2", 1, "0.000000", "-0.000000", "-0.000000", "0.000000"),
        row("c:1", "c:3", 2, "-nan", "-nan", "nan", "-nan"),
        row("c:2", "c:3", 1, "0.100000", "inf", "-inf", "0.700000"),
        row("c:2", "c:4", 2, "0.100000", "-0.000001", "0.000001", "0.000000"),
    ]) + "\n"
    # "-0.000000" reads back as -0.0, which is >= 0: it passes a signed floor of 0; a value one unit below does not
    assert names(linked_ref.linked_lines(t, field=5, min_weight=0.0, abs_value=False)) == [("c:1", "c:2")]
    assert names(linked_ref.linked_lines(t, field=5, min_weight=0.0)) == [("c:1", "c:2"), ("c:2", "c:4")]
    # nan and inf are never linked, whatever the floor: -inf signed passes every finite row and only those
    assert names(linked_ref.linked_lines(t, field=5, min_weight=-math.inf, abs_value=False)) == [("c:1", "c:2"), ("c:2", "c:4")]
    assert names(linked_ref.linked_lines(t, field=6, min_weight=-math.inf, abs_value=False)) == [("c:1", "c:2"), ("c:2", "c:4")]
    assert names(linked_ref.linked_lines(t, field=7, min_weight=-math.inf)) == [("c:1", "c:2"), ("c:2", "c:3"), ("c:2", "c:4")]
    assert linked_ref.linked_lines(t, field=4, min_weight=math.inf) == []


def test_rows_across_chromosomes_and_the_limit():
    t = HEAD + "\n".join([
        row("a:100", "a:1100", 1000, "0.6", "0.1", "1.0", "0.600000"),
        row("a:100", "a:1101", 1001, "0.6", "0.1", "1.0", "0.600000"),
        row("a:100", "b:50", "inf", "0.6", "0.1", "1.0", "0.900000"),
        row("a:1100", "b:50", "inf", "0.6", "0.1", "1.0", "0.100000"),
    ]) + "\n"
    # no limit: no condition on dist at all -- the row across chromosomes is there if its value is
    assert names(linked_ref.linked_lines(t)) == [("a:100", "a:1100"), ("a:100", "a:1101"), ("a:100", "b:50")]
    # a finite limit: dist finite and <= limit * 1000, not strict
    assert names(linked_ref.linked_lines(t, max_kb_dist=1.0)) == [("a:100", "a:1100")]
    assert names(linked_ref.linked_lines(t, max_kb_dist=1.5)) == [("a:100", "a:1100"), ("a:100", "a:1101")]
    assert names(linked_ref.linked_lines(t, max_kb_dist=1e300)) == [("a:100", "a:1100"), ("a:100", "a:1101")]
    assert linked_ref.linked_lines(t, max_kb_dist=0.0) == []


def test_maf_at_equality_nan_maf_extra_label_columns_and_plain_tables():
    t = HEAD + "\n".join([
        row("c:1", "c:2", 1, "0.6", "0.1", "1.0", "0.600000", maf1="0.125000", maf2="0.300000"),
        row("c:1", "c:3", 2, "0.6", "0.1", "1.0", "0.600000", maf1="0.125000", maf2="0.124999"),
        row("c:2", "c:4", 2, "0.6", "0.1", "1.0", "0.600000", maf1="0.300000", maf2="-nan"),
    ]) + "\n"
    assert names(linked_ref.linked_lines(t, min_maf=0.125)) == [("c:1", "c:2")]
    assert names(linked_ref.linked_lines(t, min_maf=0.124999)) == [("c:1", "c:2"), ("c:1", "c:3")]
    assert names(linked_ref.linked_lines(t)) == [("c:1", "c:2"), ("c:1", "c:3")]  # (a NaN maf never passes, even at 0)
    # labels that carry a second column: every field lies two places further on
    wide = "\n".join([
        row("c:1\tx", "c:2\ty", 1, "0.6", "0.1", "1.0", "0.600000"),
        row("c:1\tx", "c:3\tz", 2, "0.6", "0.1", "1.0", "0.400000"),
    ]) + "\n"
    got = linked_ref.linked_lines(wide, label_cols=2)
    assert got == wide.splitlines()[:1]
    # the table without the extended columns: the maf by label
    plain = "c:1\tc:2\t1\t0.6\t0.1\t1.0\t0.600000\nc:1\tc:3\t2\t0.6\t0.1\t1.0\t0.700000\n"
    maf = {"c:1": 0.2, "c:2": 0.1, "c:3": float("nan")}
    assert linked_ref.linked_lines(plain, maf=maf, min_maf=0.1) == plain.splitlines()[:1]
    with pytest.raises(ValueError):
        linked_ref.linked_lines(plain)
