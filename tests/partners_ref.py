"""The rule of PARTNERS.md in plain Python, over an ngsLD TSV plus the site indices (s1, s2) of its rows: every site's partner
rows, ranked, cut to k.

Every value becomes an integer of micro-units from the row's own text by stripping the point ("%f" always prints six decimals):
no float takes part in a value or in the ranking.  The floor is compared as the rule states it, q / 10^6 >= min_weight as doubles
(Python's int / int is correctly rounded).  The maf comes from the --extend_out columns (maf1, maf2); a table without them needs
`maf`, the printed maf of every label, as tests/linked_ref.py does."""
import math

import numpy as np

# TSV column (1-based, as --partners_field counts) -> its place after the two labels and dist
FIELDS = {4: 1, 5: 2, 6: 3, 7: 4}
NAMES = {4: "r2_ExpG", 5: "D", 6: "Dp", 7: "r2"}
Q_LIMIT = 1 << 31


class RangeError(ValueError):
    """A finite value of 2^31 micro-units or more in a row that passes the maf and distance tests (rule 4); .pair = (s1, s2)."""

    def __init__(self, pair):
        super().__init__(f"pair {pair[0]} - {pair[1]} reaches 2^31 micro-units")
        self.pair = pair


def micro(txt: str):
    """The "%f" text of a value as integer micro-units; None for nan / inf.  "-0.000000" is 0."""
    t = txt.strip().lower()
    if "nan" in t or "inf" in t:
        return None
    whole, frac = t.split(".")
    assert len(frac) == 6 and frac.isdigit(), txt
    neg = whole.startswith("-")
    q = int(whole.lstrip("+-") + frac)
    return -q if neg else q


def rows_of(text: str) -> list[str]:
    return [ln for ln in text.splitlines() if ln and not ln.startswith("site1\t")]


def partners(text: str, s1, s2, n_sites: int, k: int, field: int = 7, min_weight: float = 0.5, abs_value: bool = True,
             max_kb_dist: float = math.inf, min_maf: float = 0.0, query=None, label_cols: int = 1, maf: dict | None = None):
    """(rows uint64[n], partner int64[n, k] with -1 for none, value_micro int64[n, k] with 0 for none): row j of `text` is the
    pair (s1[j], s2[j]).  query: None, or one entry per site, a site collects partners iff its entry is not 0."""
    if field not in FIELDS:
        raise ValueError("field must be a TSV column 4..7")
    if not 1 <= k <= 64:
        raise ValueError("k must be in 1..64")
    lines = rows_of(text)
    assert len(lines) == len(s1) == len(s2)
    base = 2 * label_cols  # (the dist column)
    found = [[] for _ in range(n_sites)]  # per site: (-q, partner)
    for ln, a, b in zip(lines, s1, s2):
        a, b = int(a), int(b)
        f = ln.split("\t")
        q = micro(f[base + FIELDS[field]])
        if q is None:
            continue
        if len(f) > base + 5:
            maf1, maf2 = float(f[base + 6]), float(f[base + 7])
        else:
            if maf is None:
                raise ValueError("a table without the extended columns needs the sites' maf")
            maf1, maf2 = maf["\t".join(f[:label_cols])], maf["\t".join(f[label_cols:base])]
        if not (maf1 >= min_maf and maf2 >= min_maf):  # (a NaN maf never passes)
            continue
        if math.isfinite(max_kb_dist):  # (the default: no condition on dist at all)
            dist = float(f[base])
            if not (math.isfinite(dist) and dist <= max_kb_dist * 1000):
                continue
        if abs(q) >= Q_LIMIT:
            raise RangeError((a, b))
        if abs_value:
            q = abs(q)
        if not q / 10 ** 6 >= min_weight:
            continue
        if query is None or query[a]:
            found[a].append((-q, b))
        if query is None or query[b]:
            found[b].append((-q, a))
    rows = np.zeros(n_sites, dtype=np.uint64)
    partner = np.full((n_sites, k), -1, dtype=np.int64)
    value = np.zeros((n_sites, k), dtype=np.int64)
    for s, lst in enumerate(found):
        rows[s] = len(lst)
        for j, (nq, p) in enumerate(sorted(lst)[:k]):
            partner[s, j] = p
            value[s, j] = -nq
    return rows, partner, value


def micro_text(q: int) -> str:
    a = abs(int(q))
    return f"{'-' if q < 0 else ''}{a // 10 ** 6}.{a % 10 ** 6:06d}"


def partners_file(partner, value_micro, names, field: int = 7) -> str:
    """The file --partners_out writes: the header, then one line per kept partner in site order, then rank order from 1.
    names[s]: the site as the binary names it (its label up to the first TAB; without --pos its 1-based index)."""
    out = [f"site\trank\tpartner\t{NAMES[field]}\n"]
    for s in range(len(partner)):
        for j, p in enumerate(partner[s]):
            if p < 0:
                break
            out.append(f"{names[s]}\t{j + 1}\t{names[int(p)]}\t{micro_text(value_micro[s][j])}\n")
    return "".join(out)
