"""Plain Python restatement of LD across chromosomes (CROSS.md) over the TSV text ngsLD writes -- the yardstick of
ngsld_cross_ld, the way grid_ref.py is of ngsld_grid.

* every value is what the TSV prints, read back: the decimal text of a "%f" column becomes an integer of micro-units with int
  alone (site_ref.micro), "%.0f" dist an int; |q| with abs_value;
* a site's chromosome and position come from its label "CHR:pos"; bin = pos // bin_size, 0 with bin_size 0 (one bin per
  chromosome); the bins are numbered consecutively over the chromosomes in file order, each chromosome from the bin of its first
  site to the bin of its last;
* a row counts iff maf1 >= min_maf and maf2 >= min_maf (only where the file has those columns -- --extend_out; a NaN maf never
  passes), every chosen statistic is finite, and either its dist is not finite (two chromosomes) or `within` holds and
  dist >= min_kb_dist * 1000;
* a counted row adds to ONE cell, (chr1, bin(site1), chr2, bin(site2)): n, per statistic sum and max of q, linked = rows with
  q / 10^6 >= linked_min (a comparison of doubles: int / int is the printed value read back);
* mean = float(Fraction(sum, 10^6 * n)), the one rounding; only cells with rows exist, ordered by the consecutive bin of site1,
  then of site2.
"""
from __future__ import annotations

from fractions import Fraction

from site_ref import COLUMNS, FIELDS, MICRO, micro, micro_text, printed


def _chr_pos(label: str) -> tuple[str, int]:
    name, _, num = label.partition(":")
    assert num.isdigit() and num.isascii(), label
    return name, int(num)


def gbins(sites: list[str], bin_size: int) -> dict:
    """label -> (consecutive bin, chromosome, bin): a chromosome is a run of equal names in file order."""
    out, g0, prev = {}, 0, None
    first = last = 0
    for lab in sites:
        name, pos = _chr_pos(lab)
        b = pos // bin_size if bin_size else 0
        if name != prev:
            assert all(v[1] != name for v in out.values()), f"chromosome {name} begins twice"
            if prev is not None:
                g0 += last - first + 1
            first, prev = b, name
        assert b >= first
        last = b
        out[lab] = (g0 + b - first, name, b)
    return out


def cross(text: str, sites: list[str], bin_size: int = 0, ld=("r2",), min_maf: float = 0.0, linked_min: float = 0.5,
          abs_value: bool = True, within: bool = True, min_kb_dist: float = 0.0) -> dict:
    """{"chr1": [..], "bin1": [..], "chr2": [..], "bin2": [..], "n": [..], "sum_F": [..], "max_F": [..], "linked_F": [..],
    "mean_F": [..]} per statistic F of ld in TSV column order, one entry per cell with rows; bin1 and bin2 are the windows' lower
    breaks b * bin_size (0 with bin_size 0)."""
    assert isinstance(bin_size, int) and 0 <= bin_size < 2 ** 31
    where = gbins(sites, bin_size)
    lines = [ln for ln in text.splitlines() if ln]
    if lines and lines[0].startswith("site1\t"):
        head = lines.pop(0).split("\t")
    else:
        head = COLUMNS[:7] if not lines or len(lines[0].split("\t")) == 7 else COLUMNS
    col = {name: k for k, name in enumerate(head)}
    chosen = [f for f in FIELDS if f in ld]
    assert chosen
    floor = min_kb_dist * 1000
    cells = {}
    for ln in lines:
        f = ln.split("\t")
        (g1, c1, b1), (g2, c2, b2) = where[f[col["site1"]]], where[f[col["site2"]]]
        dist = f[col["dist"]].strip()
        if dist.lstrip("+-").lower() in ("inf", "nan"):
            assert c1 != c2, ln  # (a dist that is not finite: two chromosomes)
        else:
            assert c1 == c2, ln
            if not within or not int(dist) >= floor:
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
        assert g1 <= g2, ln
        cell = cells.setdefault((g1, g2, c1, b1, c2, b2), {"n": 0, "sum": [0] * len(qs), "max": list(qs), "linked": [0] * len(qs)})
        cell["n"] += 1
        for k, q in enumerate(qs):
            cell["sum"][k] += q
            cell["max"][k] = max(cell["max"][k], q)
            if printed(q) >= linked_min:
                cell["linked"][k] += 1
    keys = sorted(cells)
    out = {"chr1": [k[2] for k in keys], "bin1": [k[3] * bin_size for k in keys], "chr2": [k[4] for k in keys],
           "bin2": [k[5] * bin_size for k in keys], "n": [cells[k]["n"] for k in keys]}
    for j, name in enumerate(chosen):
        out[f"sum_{name}"] = [cells[k]["sum"][j] for k in keys]
        out[f"max_{name}"] = [cells[k]["max"][j] for k in keys]
        out[f"linked_{name}"] = [cells[k]["linked"][j] for k in keys]
        out[f"mean_{name}"] = [float(Fraction(cells[k]["sum"][j], MICRO * cells[k]["n"])) for k in keys]
    return out


def cross_file(text: str, sites: list[str], bin_size: int = 0, **kw) -> str:
    """The --cross_out file of the TSV: header, then one line per cell with rows."""
    res = cross(text, sites, bin_size, **kw)
    chosen = [f for f in FIELDS if f in kw.get("ld", ("r2",))]
    rows = ["\t".join(["chr1", "bin1", "chr2", "bin2", "n"] + [f"{w}_{f}" for f in chosen for w in ("sum", "mean", "max", "linked")])]
    for i in range(len(res["n"])):
        cells = [res["chr1"][i], str(res["bin1"][i]), res["chr2"][i], str(res["bin2"][i]), str(res["n"][i])]
        for f in chosen:
            cells += [micro_text(res[f"sum_{f}"][i]), "%.17g" % res[f"mean_{f}"][i], micro_text(res[f"max_{f}"][i]),
                      str(res[f"linked_{f}"][i])]
        rows.append("\t".join(cells))
    return "\n".join(rows) + "\n"
