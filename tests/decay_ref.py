"""Plain Python restatement of the reference's LD decay binning (scripts/fit_LDdecay.R v1.1.0, its default mean bins, one LD
file) over the TSV text ngsLD writes -- the yardstick of ngsld_decay, the way prune_ref.py is of ngsld_prune.  DECAY.md has
the rule.

* every value is what the TSV prints, read back (float() of the text; "-nan" / "inf" as R reads them);
* a row is kept iff maf1 >= min_maf and maf2 >= min_maf (only where the file has those columns, as in the script), and
  dist < max_kb_dist * 1000 (strict; a dist that is not finite never passes);
* a row with NaN or +-inf in any chosen statistic drops out of every one (Inf -> NA, then aggregate's na.omit);
* breaks = seq(0, max(dist) + B, B) (k * B, the last one clipped), bins right-closed (b_k, b_k+1], labelled with the lower
  break through as.character (15 significant digits); empty bins do not appear;
* a bin's value is the mean of its rows' printed values -- exact here, as a Fraction of the decimal texts.

The fit (section 7 of the rule) is stated by model() and sse() below; tests/test_decay_host.py holds the library's fit to a
bounded multi-start minimiser of the same sum of squares.
"""
from __future__ import annotations

import bisect
import math
from fractions import Fraction

FIELDS = ("r2_ExpG", "D", "Dp", "r2")
COLUMNS = ["site1", "site2", "dist", "r2_ExpG", "D", "Dp", "r2", "sample_size", "maf1", "maf2", "hap00", "hap01", "hap10", "hap11",
           "hap_maf1", "hap_maf2", "chi2", "loglike", "nIter"]


def r_seq(frm: float, to: float, by: float) -> list[float]:
    """R's seq(from, to, by) for by > 0: from + (0:n) * by, n = floor((to - from) / by + 1e-10), clipped to `to`."""
    n = int(math.floor((to - frm) / by + 1e-10))
    return [min(frm + k * by, to) for k in range(n + 1)]


def decay_bins(text: str, ld=("r2",), bin_size: float = 250, max_kb_dist: float = math.inf, min_maf: float = 0.0):
    """[(dist, n, {stat: Fraction mean})] of an ngsLD TSV (header line included), in increasing dist; stats in TSV column
    order, whatever the order of ld."""
    assert bin_size > 1
    lines = [ln for ln in text.splitlines() if ln]
    if lines and lines[0].startswith("site1\t"):
        head = lines.pop(0).split("\t")
    else:  # (rows without their header: ngsLD's column layout, standard or --extend_out)
        head = COLUMNS[:7] if not lines or len(lines[0].split("\t")) == 7 else COLUMNS
    col = {name: k for k, name in enumerate(head)}
    chosen = [f for f in FIELDS if f in ld]
    limit = max_kb_dist * 1000
    rows = []  # (dist, [texts]) of the rows that pass the maf and distance filters
    for ln in lines:
        f = ln.split("\t")
        if "maf1" in col and "maf2" in col and not (float(f[col["maf1"]]) >= min_maf and float(f[col["maf2"]]) >= min_maf):
            continue
        dist = float(f[col["dist"]])
        if not dist < limit:
            continue
        rows.append((dist, [f[col[s]] for s in chosen]))
    if not rows:
        return []
    breaks = r_seq(0.0, max(d for d, _ in rows) + bin_size, bin_size)
    acc: dict[int, list] = {}
    for dist, texts in rows:
        vals = [float(t) for t in texts]
        if any(not math.isfinite(v) for v in vals):
            continue
        i = bisect.bisect_left(breaks, dist)  # breaks[i-1] < dist <= breaks[i]
        if i == 0 or i >= len(breaks):
            continue  # (dist <= 0: in no bin)
        a = acc.setdefault(i - 1, [0] + [Fraction(0)] * len(chosen))
        a[0] += 1
        for k, t in enumerate(texts):
            a[k + 1] += Fraction(t)
    out = []
    for b in sorted(acc):
        a = acc[b]
        out.append((float(f"{breaks[b]:.15g}"), a[0], {s: a[k + 1] / a[0] for k, s in enumerate(chosen)}))
    return out


def model(field: str, rate: float, h: float, l: float, d, n_ind: float = 0, recomb_rate: float = 1.0):
    """The script's ld_exp (d may be a numpy array)."""
    if field == "Dp":
        return l + (h - l) * 1.0 * (1 - d * recomb_rate / 1e6) ** rate
    C = rate * d
    if n_ind:
        return ((10 + C) / ((2 + C) * (11 + C))) * (1 + ((3 + C) * (12 + 12 * C + C * C)) / (n_ind * (2 + C) * (11 + C)))
    return (h - l) / (1 + C) + l


def sse(field: str, par, d, y, n_ind: float = 0, recomb_rate: float = 1.0) -> float:
    """The script's fit_eval: the sum of squares of the model at par = (rate, h, l) against the bin values y."""
    import numpy as np
    r = model(field, par[0], par[1], par[2], np.asarray(d, dtype=float), n_ind, recomb_rate) - np.asarray(y, dtype=float)
    return float(np.sum(r * r))
