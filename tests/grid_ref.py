"""Plain Python restatement of the LD grid (GRID.md) over the TSV text ngsLD writes -- the yardstick of ngsld_grid, the way
site_ref.py is of ngsld_site_ld.

* every value is what the TSV prints, read back: the decimal text of a "%f" column becomes an integer of micro-units with int
  alone (site_ref.micro), "%.0f" dist an int; |q| with abs_value;
* a row counts iff dist is finite and dist <= max_kb_dist * 1000, maf1 >= min_maf and maf2 >= min_maf (only where the file has
  those columns -- --extend_out; a NaN maf never passes), and every chosen statistic is finite;
* a site's chromosome and position come from its label "CHR:pos" (the text up to the first ":" and the decimal digits behind
  it); bin = pos // bin_size;
* a counted row adds to ONE cell, (chromosome, bin(site1), bin(site2)): n, per statistic sum and max of q, linked = rows with
  q / 10^6 >= linked_min (a comparison of doubles: int / int is the printed value read back);
* mean = float(Fraction(sum, 10^6 * n)), the one rounding; only cells with rows exist, ordered by chromosome (the order of
  `sites`, the labels of the input in file order), bin1, bin2.
"""
from __future__ import annotations

import math
from fractions import Fraction

from site_ref import COLUMNS, FIELDS, MICRO, micro, micro_text, printed


def _chr_pos(label: str) -> tuple[str, int]:
    name, _, num = label.partition(":")
    assert num.isdigit() and num.isascii(), label
    return name, int(num)


def grid(text: str, sites: list[str], bin_size: int, ld=("r2",), max_kb_dist: float = math.inf, min_maf: float = 0.0,
         linked_min: float = 0.5, abs_value: bool = True) -> dict:
    """{"chr": [..], "bin1": [..], "bin2": [..], "n": [..], "sum_F": [..], "max_F": [..], "linked_F": [..], "mean_F": [..]} per
    statistic F of ld in TSV column order, one entry per cell with rows; bin1 and bin2 are the windows' lower breaks b * bin_size."""
    assert isinstance(bin_size, int) and 1 <= bin_size < 2 ** 31
    where = {lab: _chr_pos(lab) for lab in sites}  # (two sites at one position share a label, and a bin)
    order = {}
    for lab in sites:
        order.setdefault(where[lab][0], len(order))
    lines = [ln for ln in text.splitlines() if ln]
    if lines and lines[0].startswith("site1\t"):
        head = lines.pop(0).split("\t")
    else:
        head = COLUMNS[:7] if not lines or len(lines[0].split("\t")) == 7 else COLUMNS
    col = {name: k for k, name in enumerate(head)}
    chosen = [f for f in FIELDS if f in ld]
    assert chosen
    limit = max_kb_dist * 1000
    cells = {}
    for ln in lines:
        f = ln.split("\t")
        dist = f[col["dist"]].strip()
        if dist.lstrip("+-").lower() in ("inf", "nan") or not int(dist) <= limit:
            continue
        if "maf1" in col and "maf2" in col:
            mafs = [micro(f[col["maf1"]]), micro(f[col["maf2"]])]
            if any(q is None or not printed(q) >= min_maf for q in mafs):
                continue
        qs = [micro(f[col[s]]) for s in chosen]
        if any(q is None for q in qs):
            continue
        if abs_value:
            qs = [abs(q) for q in qs]
        (c1, p1), (c2, p2) = where[f[col["site1"]]], where[f[col["site2"]]]
        assert c1 == c2, ln  # (a finite dist: one chromosome)
        cell = cells.setdefault((order[c1], c1, p1 // bin_size, p2 // bin_size), {"n": 0, "sum": [0] * len(qs), "max": list(qs),
                                                                                  "linked": [0] * len(qs)})
        cell["n"] += 1
        for k, q in enumerate(qs):
            cell["sum"][k] += q
            cell["max"][k] = max(cell["max"][k], q)
            if printed(q) >= linked_min:
                cell["linked"][k] += 1
    keys = sorted(cells)
    out = {"chr": [k[1] for k in keys], "bin1": [k[2] * bin_size for k in keys], "bin2": [k[3] * bin_size for k in keys],
           "n": [cells[k]["n"] for k in keys]}
    for j, name in enumerate(chosen):
        out[f"sum_{name}"] = [cells[k]["sum"][j] for k in keys]
        out[f"max_{name}"] = [cells[k]["max"][j] for k in keys]
        out[f"linked_{name}"] = [cells[k]["linked"][j] for k in keys]
        out[f"mean_{name}"] = [float(Fraction(cells[k]["sum"][j], MICRO * cells[k]["n"])) for k in keys]
    return out


def grid_file(text: str, sites: list[str], bin_size: int, **kw) -> str:
    """The --grid_out file of the TSV: header, then one line per cell with rows."""
    res = grid(text, sites, bin_size, **kw)
    chosen = [f for f in FIELDS if f in kw.get("ld", ("r2",))]
    rows = ["\t".join(["chr", "bin1", "bin2", "n"] + [f"{w}_{f}" for f in chosen for w in ("sum", "mean", "max", "linked")])]
    for i in range(len(res["n"])):
        cells = [res["chr"][i], str(res["bin1"][i]), str(res["bin2"][i]), str(res["n"][i])]
        for f in chosen:
            cells += [micro_text(res[f"sum_{f}"][i]), "%.17g" % res[f"mean_{f}"][i], micro_text(res[f"max_{f}"][i]),
                      str(res[f"linked_{f}"][i])]
        rows.append("\t".join(cells))
    return "\n".join(rows) + "\n"
