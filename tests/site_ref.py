"""Plain Python restatement of the per-site LD summaries (SITES.md) over the TSV text ngsLD writes -- the yardstick of
ngsld_site_ld, the way decay_ref.py is of ngsld_decay.

* every value is what the TSV prints, read back: the decimal text of a "%f" column becomes an integer of micro-units with int
  alone (micro), "%.0f" dist an int; |q| with abs_value;
* a row counts iff dist is finite and dist <= max_kb_dist * 1000, maf1 >= min_maf and maf2 >= min_maf (only where the file has
  those columns; a NaN maf never passes), and every chosen statistic is finite;
* a counted row adds to BOTH of its sites: n, per statistic sum and max of q, linked = rows with q / 10^6 >= linked_min;
* the comparisons with min_maf and linked_min are comparisons of doubles: the printed value read back is q / 10^6 rounded once,
  which is what Python's int / int gives (printed);
* mean = float(Fraction(sum, 10^6 * n)), the one rounding; a site without counted rows has sum 0, linked 0, mean and max None.
"""
from __future__ import annotations

import math
from fractions import Fraction

FIELDS = ("r2_ExpG", "D", "Dp", "r2")
COLUMNS = ["site1", "site2", "dist", "r2_ExpG", "D", "Dp", "r2", "sample_size", "maf1", "maf2", "hap00", "hap01", "hap10", "hap11",
           "hap_maf1", "hap_maf2", "chi2", "loglike", "nIter"]
MICRO = 10 ** 6


def micro(text: str) -> int | None:
    """"%f" text -> micro-units; None for nan / inf of either sign."""
    t = text.strip()
    neg = t.startswith("-")
    body = t.lstrip("+-")
    if body.lower() in ("nan", "inf"):
        return None
    whole, frac = body.split(".")
    assert len(frac) == 6 and whole.isdigit() and frac.isdigit(), text
    q = int(whole) * MICRO + int(frac)
    return -q if neg else q


def printed(q: int) -> float:
    """The double a reader gets from the text of q micro-units (int / int is correctly rounded)."""
    return q / MICRO


def micro_text(q: int) -> str:
    a = abs(q)
    return f"{'-' if q < 0 else ''}{a // MICRO}.{a % MICRO:06d}"


def site_ld(text: str, sites: list[str], ld=("r2",), max_kb_dist: float = math.inf, min_maf: float = 0.0,
            linked_min: float = 0.5, abs_value: bool = True) -> dict:
    """{"n": [..], "sum_F": [..], "max_F": [..], "linked_F": [..], "mean_F": [..]} per statistic F of ld in TSV column order,
    one entry per site of `sites` (the labels of the input, in file order)."""
    index = {lab: k for k, lab in enumerate(sites)}
    assert len(index) == len(sites), "site labels must be unique"
    lines = [ln for ln in text.splitlines() if ln]
    if lines and lines[0].startswith("site1\t"):
        head = lines.pop(0).split("\t")
    else:
        head = COLUMNS[:7] if not lines or len(lines[0].split("\t")) == 7 else COLUMNS
    col = {name: k for k, name in enumerate(head)}
    chosen = [f for f in FIELDS if f in ld]
    assert chosen
    m = len(sites)
    out = {"n": [0] * m}
    for f in chosen:
        out[f"sum_{f}"], out[f"max_{f}"], out[f"linked_{f}"] = [0] * m, [None] * m, [0] * m
    limit = max_kb_dist * 1000
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
        ends = (index[f[col["site1"]]], index[f[col["site2"]]])
        assert ends[0] != ends[1]
        for s in ends:
            out["n"][s] += 1
            for name, q in zip(chosen, qs):
                out[f"sum_{name}"][s] += q
                top = out[f"max_{name}"][s]
                out[f"max_{name}"][s] = q if top is None else max(top, q)
                if printed(q) >= linked_min:
                    out[f"linked_{name}"][s] += 1
    for name in chosen:
        out[f"mean_{name}"] = [float(Fraction(t, MICRO * n)) if n else None for t, n in zip(out[f"sum_{name}"], out["n"])]
    return out


def site_file(text: str, sites: list[str], names: list[str] | None = None, **kw) -> str:
    """The --site_out file of the TSV: header, then one line per site (names: the first column, default the labels)."""
    res = site_ld(text, sites, **kw)
    chosen = [f for f in FIELDS if f in kw.get("ld", ("r2",))]
    rows = ["\t".join(["site", "n"] + [f"{w}_{f}" for f in chosen for w in ("sum", "mean", "max", "linked")])]
    for s, lab in enumerate(names if names is not None else sites):
        cells = [lab, str(res["n"][s])]
        for f in chosen:
            mean, top = res[f"mean_{f}"][s], res[f"max_{f}"][s]
            cells += [micro_text(res[f"sum_{f}"][s]), "NA" if mean is None else "%.17g" % mean,
                      "NA" if top is None else micro_text(top), str(res[f"linked_{f}"][s])]
        rows.append("\t".join(cells))
    return "\n".join(rows) + "\n"
