"""Plain Python restatement of the LD decay map (ngsld_decay_map, DECAY_MAP.md) over the TSV text ngsLD writes: the rows of the
table are split into groups and tests/decay_ref.py -- the restatement of fit_LDdecay.R's binning for one LD file -- is applied to
each group's rows under the table's header, exactly as a user splits the table by chromosome or region and gives the script one
file per part.

* a row's group comes from its two labels CHR:pos alone: rows whose sites lie on two chromosomes are dropped;
* window 0: the group is the chromosome, win_start 0;
* window W: the group is (chromosome, w) with w = (p1 + p2) // (2 * W) in integer arithmetic -- the window that holds the pair's
  midpoint, which may hold neither site -- and win_start = w * W;
* groups are listed in the order their chromosome first appears in the table, then w ascending, and only groups with a bin.
"""
from __future__ import annotations

import math

import decay_ref


def split_rows(text: str, window: int = 0):
    """(header line or None, {(chr, w): [row lines]}, [chr in order of first appearance])."""
    assert window == int(window) and window >= 0
    lines = [ln for ln in text.splitlines() if ln]
    head = lines.pop(0) if lines and lines[0].startswith("site1\t") else None
    groups: dict[tuple[str, int], list[str]] = {}
    order: list[str] = []
    for ln in lines:
        a, b = ln.split("\t")[:2]
        c1, p1 = a.split(":", 1)
        c2, p2 = b.split(":", 1)
        if c1 != c2:
            continue
        if c1 not in order:
            order.append(c1)
        w = (int(p1) + int(p2)) // (2 * int(window)) if window else 0
        groups.setdefault((c1, w), []).append(ln)
    return head, groups, order


def decay_map(text: str, window: int = 0, ld=("r2",), bin_size: float = 250, max_kb_dist: float = math.inf, min_maf: float = 0.0):
    """[(chr, win_start, bins)] with bins what decay_ref.decay_bins gives for the group's rows; groups without a bin are left out."""
    head, groups, order = split_rows(text, window)
    out = []
    for c, w in sorted(groups, key=lambda g: (order.index(g[0]), g[1])):
        part = "\n".join(([head] if head else []) + groups[(c, w)]) + "\n"
        bins = decay_ref.decay_bins(part, ld=ld, bin_size=bin_size, max_kb_dist=max_kb_dist, min_maf=min_maf)
        if bins:
            out.append((c, w * int(window), bins))
    return out
