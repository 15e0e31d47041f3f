"""Plain Python restatement of the reference's LD block matrices (scripts/LD_blocks.sh) over the TSV text ngsLD writes -- the
yardstick of ngsld_blocks, the way decay_ref.py is of ngsld_decay.  BLOCKS.md has the rule.

* the script's awk filter: a row is in the region iff both labels split on ":" give CHR and a position p with
  START <= p <= END (both inclusive); its `cut -f 1-7` keeps site1, site2, dist, r2_ExpG, D, Dp, r2;
* the TSV's "site1\\tsite2\\t..." header line is not a pair: skipped whether or not the text has one;
* a label is a member candidate iff the text before its first ":" is CHR byte for byte; its position part must be plain
  decimal digits, and two members may not share a numeric position (acast would merge them): both are refused, as is a
  "(null)" label (no positions);
* the matrix sites are unique(c(snp1, snp2)) of the in-region rows in increasing position (mixedorder on labels that share
  CHR:), every one both a row and a column;
* cell [snp1][snp2] is the row's text of the statistic exactly as the TSV prints it, NA elsewhere (the diagonal included);
* the file: an empty first cell and the labels, then per site its label and one cell per site, TAB separated.
"""
from __future__ import annotations

FIELDS = ("r2_ExpG", "D", "Dp", "r2")
COLUMN = {"r2_ExpG": 3, "D": 4, "Dp": 5, "r2": 6}  # of the cut -f 1-7 fields


class Refused(ValueError):
    """What the library refuses: kind "invalid" (no positions) or "unsupported" (a bad or repeated position)."""

    def __init__(self, kind: str, msg: str):
        super().__init__(msg)
        self.kind = kind


def _position(label: str, chr: str):
    """The label's position if it is a member candidate (chr part == CHR), else None; refuses a bad position part."""
    if label == "(null)":
        raise Refused("invalid", "LD blocks need positions: a label is \"(null)\"")
    head, colon, num = label.partition(":")
    if head != chr:
        return None
    if not num or len(num) > 19 or not all("0" <= ch <= "9" for ch in num):
        raise Refused("unsupported", f"the position of label {label!r} is not plain decimal digits")
    return int(num)


def blocks(text: str, chr: str, start: int, end: int, ld=("r2", "Dp")) -> tuple[list[str], dict, dict]:
    """(matrix site labels in matrix order, {stat: file text}, {"pairs_in_region", "sites", "members"}) of an ngsLD TSV."""
    assert start < end, "start position must be smaller than end position."
    chosen = [f for f in FIELDS if f in ld]
    assert chosen, ld
    pos = {}        # member label -> position
    rows = []       # (snp1, snp2, [7 fields]) of the in-region pairs
    for ln in text.split("\n"):
        if not ln or ln.startswith("site1\t"):
            continue
        f = ln.split("\t")[:7]
        inside = True
        for lab in f[:2]:
            p = _position(lab, chr)
            if p is not None and start <= p <= end:
                pos[lab] = p
            else:
                inside = False
        if inside:
            rows.append((f[0], f[1], f))
    by_pos = {}
    for lab, p in pos.items():
        if p in by_pos:
            raise Refused("unsupported", f"sites {by_pos[p]!r} and {lab!r} of the region share a position")
        by_pos[p] = lab
    sites = sorted({r[0] for r in rows} | {r[1] for r in rows}, key=lambda lab: pos[lab])
    at = {lab: k for k, lab in enumerate(sites)}
    files = {}
    for stat in chosen:
        cells = [["NA"] * len(sites) for _ in sites]
        for a, b, f in rows:
            cells[at[a]][at[b]] = f[COLUMN[stat]]
        out = ["".join("\t" + lab for lab in sites) + "\n"]
        for lab, row in zip(sites, cells):
            out.append(lab + "".join("\t" + c for c in row) + "\n")
        files[stat] = "".join(out)
    return sites, files, {"pairs_in_region": len(rows), "sites": len(sites), "members": len(pos)}
