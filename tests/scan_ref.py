"""Plain Python restatement of the LD scan (SCAN.md) over the TSV text ngsLD writes -- the yardstick of ngsld_scan, the way
site_ref.py is of ngsld_site_ld.  It imports nothing from the engine.

* every value is what the TSV prints, read back: the decimal text of a "%f" column becomes an integer of micro-units with int
  alone (micro), "%.0f" dist an int; the value is always |q|;
* a row counts iff dist is finite and dist <= max_kb_dist * 1000, maf1 >= min_maf and maf2 >= min_maf (only where the file has
  those columns; a NaN maf never passes), and every chosen statistic is finite;
* the window of a site c is the index range [a_c, b_c] of the sites on c's chromosome -- a run of labels with one CHR -- whose
  position is within half_window of c's (windows); its left flank is [a_c, c], its right flank [c + 1, b_c];
* a counted row (i, j), i < j, is in window c iff a_c <= i and j <= b_c: LL if j <= c, RR if i > c, LR otherwise;
* per site: n_ll, n_rr, n_lr and per statistic the sums of q by class; zns = float(Fraction(S, 10^6 * n)) over all three
  classes, omega = float(Fraction((S_LL + S_RR) * n_LR, (n_LL + n_RR) * S_LR)); None where the denominator is 0.

scan_brute applies the definition window by window; scan adds each row to the ranges of windows it is in (SCAN.md, "the
decomposition") and is what the GPU tests use on tables of 10^5 rows.  tests/test_scan_ref.py holds the two to each other.
"""
from __future__ import annotations

import math
from fractions import Fraction

FIELDS = ("r2_ExpG", "D", "Dp", "r2")
COLUMNS = ["site1", "site2", "dist", "r2_ExpG", "D", "Dp", "r2", "sample_size", "maf1", "maf2", "hap00", "hap01", "hap10", "hap11",
           "hap_maf1", "hap_maf2", "chi2", "loglike", "nIter"]
MICRO = 10 ** 6
CLASSES = ("ll", "rr", "lr")


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


def micro_text(q: int) -> str:
    a = abs(q)
    return f"{'-' if q < 0 else ''}{a // MICRO}.{a % MICRO:06d}"


def positions_of(sites: list[str]) -> list[tuple[str, int]]:
    """(CHR, pos) of labels CHR:pos (up to the first TAB)."""
    out = []
    for lab in sites:
        chrom, _, pos = lab.split("\t")[0].partition(":")
        out.append((chrom, int(pos)))
    return out


def windows(positions: list[tuple[str, int]] | None, n: int, half_window: int) -> tuple[list[int], list[int]]:
    """(a, b): the window of site c is [a[c], b[c]].  positions None (no --pos): every dist is infinite, a window is its site."""
    if positions is None:
        return list(range(n)), list(range(n))
    assert len(positions) == n
    a, b = [0] * n, [0] * n
    for c in range(n):
        lo = c
        while lo > 0 and positions[lo - 1][0] == positions[c][0] and positions[c][1] - positions[lo - 1][1] <= half_window:
            lo -= 1
        hi = c
        while hi + 1 < n and positions[hi + 1][0] == positions[c][0] and positions[hi + 1][1] - positions[c][1] <= half_window:
            hi += 1
        a[c], b[c] = lo, hi
    return a, b


def counted_rows(text: str, sites: list[str], ld=("r2",), max_kb_dist: float = math.inf, min_maf: float = 0.0) -> list[tuple]:
    """The rows that count, as (i, j, (q of every chosen statistic in TSV column order)) with i < j site indices."""
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
    limit = max_kb_dist * 1000
    rows = []
    for ln in lines:
        f = ln.split("\t")
        dist = f[col["dist"]].strip()
        if dist.lstrip("+-").lower() in ("inf", "nan") or not int(dist) <= limit:
            continue
        if "maf1" in col and "maf2" in col:
            mafs = [micro(f[col["maf1"]]), micro(f[col["maf2"]])]
            if any(q is None or not q / MICRO >= min_maf for q in mafs):
                continue
        qs = [micro(f[col[s]]) for s in chosen]
        if any(q is None for q in qs):
            continue
        i, j = index[f[col["site1"]]], index[f[col["site2"]]]
        assert i < j
        rows.append((i, j, tuple(abs(q) for q in qs)))
    return rows


def class_of(i: int, j: int, c: int) -> int:
    """0 LL, 1 RR, 2 LR of a row (i, j) in window c."""
    return 0 if j <= c else 1 if i > c else 2


def ranges_of(i: int, j: int, a: list[int], b: list[int]) -> list[tuple[int, int]]:
    """The windows a row (i, j) is in, by class: inclusive (first, last) centre sites for LL, RR, LR; first > last: none."""
    return [(j, b[i]), (a[j], i - 1), (max(a[j], i), min(b[i], j - 1))]


def _finish(n, ns, cnt, sums, a, b, chosen):
    out = {"win_first": list(a), "win_last": list(b)}
    for k, cl in enumerate(CLASSES):
        out[f"n_{cl}"] = cnt[k]
    for v, f in enumerate(chosen):
        for k, cl in enumerate(CLASSES):
            out[f"sum_{cl}_{f}"] = sums[k][v]
        zns, omega = [None] * n, [None] * n
        for c in range(n):
            n_ll, n_rr, n_lr = cnt[0][c], cnt[1][c], cnt[2][c]
            s_ll, s_rr, s_lr = sums[0][v][c], sums[1][v][c], sums[2][v][c]
            if n_ll + n_rr + n_lr:
                zns[c] = float(Fraction(s_ll + s_rr + s_lr, MICRO * (n_ll + n_rr + n_lr)))
            if n_ll + n_rr and n_lr and s_lr:
                omega[c] = float(Fraction((s_ll + s_rr) * n_lr, (n_ll + n_rr) * s_lr))
        out[f"zns_{f}"], out[f"omega_{f}"] = zns, omega
    return out


def scan_rows(rows: list[tuple], a: list[int], b: list[int], chosen: list[str], brute: bool = False) -> dict:
    n, ns = len(a), len(chosen)
    cnt = [[0] * (n + 1) for _ in CLASSES]
    sums = [[[0] * (n + 1) for _ in range(ns)] for _ in CLASSES]
    if brute:  # the definition, window by window
        for i, j, qs in rows:
            for c in range(n):
                if a[c] <= i and j <= b[c]:
                    k = class_of(i, j, c)
                    cnt[k][c] += 1
                    for v in range(ns):
                        sums[k][v][c] += qs[v]
    else:  # every row into the ranges of windows it is in, as differences; one running sum at the end
        for i, j, qs in rows:
            for k, (x, y) in enumerate(ranges_of(i, j, a, b)):
                if x > y:
                    continue
                cnt[k][x] += 1
                cnt[k][y + 1] -= 1
                for v in range(ns):
                    sums[k][v][x] += qs[v]
                    sums[k][v][y + 1] -= qs[v]
        for arr in cnt + [s for per in sums for s in per]:
            run = 0
            for c in range(n + 1):
                run += arr[c]
                arr[c] = run
            assert arr[n] == 0
    cnt = [x[:n] for x in cnt]
    sums = [[s[:n] for s in per] for per in sums]
    return _finish(n, ns, cnt, sums, a, b, chosen)


NO_POS = object()


def scan(text: str, sites: list[str], half_window: int, ld=("r2",), max_kb_dist: float = math.inf, min_maf: float = 0.0,
         positions=None, brute: bool = False, rows: list[tuple] | None = None) -> dict:
    """{"win_first", "win_last", "n_ll", "n_rr", "n_lr", and per statistic F of ld in TSV column order "sum_ll_F", "sum_rr_F",
    "sum_lr_F", "zns_F", "omega_F"}: one entry per site of `sites` (the labels of the input, in file order).  positions: the
    sites' (CHR, pos) where the labels are not CHR:pos; NO_POS for a run without positions.  rows: counted_rows of the same
    text and filters, where a caller scans one table at several half windows."""
    assert 0 <= half_window < 2 ** 31
    chosen = [f for f in FIELDS if f in ld]
    if rows is None:
        rows = counted_rows(text, sites, ld=ld, max_kb_dist=max_kb_dist, min_maf=min_maf)
    pos = None if positions is NO_POS else positions if positions is not None else positions_of(sites)
    a, b = windows(pos, len(sites), half_window)
    return scan_rows(rows, a, b, chosen, brute=brute)


def _g17(x: float | None) -> str:
    return "NA" if x is None else "%.17g" % x


def scan_file(text: str, sites: list[str], half_window: int, names: list[str] | None = None, **kw) -> str:
    """The --scan_out file of the TSV: header, then one line per site (names: the first column, default the labels up to
    their first TAB)."""
    res = scan(text, sites, half_window, **kw)
    chosen = [f for f in FIELDS if f in kw.get("ld", ("r2",))]
    head = ["site", "win_sites", "left_sites", "right_sites", "n_ll", "n_rr", "n_lr"]
    for f in chosen:
        head += [f"sum_ll_{f}", f"sum_rr_{f}", f"sum_lr_{f}", f"zns_{f}", f"omega_{f}"]
    out = ["\t".join(head)]
    for c, lab in enumerate(names if names is not None else [s.split("\t")[0] for s in sites]):
        a, b = res["win_first"][c], res["win_last"][c]
        cells = [lab, str(b - a + 1), str(c - a + 1), str(b - c)] + [str(res[f"n_{cl}"][c]) for cl in CLASSES]
        for f in chosen:
            cells += [micro_text(res[f"sum_{cl}_{f}"][c]) for cl in CLASSES] + [_g17(res[f"zns_{f}"][c]), _g17(res[f"omega_{f}"][c])]
        out.append("\t".join(cells))
    return "\n".join(out) + "\n"
