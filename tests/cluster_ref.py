"""Plain Python restatement of the LD clusters (CLUSTERS.md) over the TSV text ngsLD writes -- the yardstick of ngsld_clusters,
the way prune_ref.py is of ngsld_prune and site_ref.py of ngsld_site_ld.

* nodes: both ends of every row;
* a row is an edge iff its dist is finite and dist <= max_kb_dist * 1000, maf1 >= min_maf and maf2 >= min_maf (only where the
  file has those columns; a NaN maf never passes), the chosen column is finite and its value q micro-units -- the decimal text
  made an integer with int alone, |q| with abs_value -- has q / 10^6 >= min_weight as doubles (int / int is correctly rounded:
  the double a reader gets from the text);
* clusters: the connected components over the nodes (a dictionary union-find), numbered 1, 2, ... in increasing order of their
  smallest site index, singletons included; a site in no row has cluster 0;
* per cluster size, first, last, span = position of last - position of first (the positions are the labels' part after the
  last ":"; 0 for a singleton), edges, sum of q, mean = float(Fraction(sum, 10^6 * edges)) and
  density = float(Fraction(edges, size * (size - 1) / 2)), None where they have no value.
"""
from __future__ import annotations

import math
from fractions import Fraction

COLUMNS = ["site1", "site2", "dist", "r2_ExpG", "D", "Dp", "r2", "sample_size", "maf1", "maf2", "hap00", "hap01", "hap10", "hap11",
           "hap_maf1", "hap_maf2", "chi2", "loglike", "nIter"]
MICRO = 10 ** 6
HEADER = "cluster\tsize\tfirst\tlast\tspan\tedges\tsum\tmean\tdensity"


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


def tsv_edges(text: str, sites: list[str], field: int = 7, min_weight: float = 0.5, max_kb_dist: float = math.inf,
              min_maf: float = 0.0, abs_value: bool = True):
    """(nodes: set of site indices, edges: [(s1, s2, q)]) of an ngsLD TSV (a header line is skipped)."""
    index = {lab: k for k, lab in enumerate(sites)}
    assert len(index) == len(sites), "site labels must be unique"
    lines = [ln for ln in text.splitlines() if ln]
    if lines and lines[0].startswith("site1\t"):
        head = lines.pop(0).split("\t")
    else:
        head = COLUMNS[:7] if not lines or len(lines[0].split("\t")) == 7 else COLUMNS
    col = {name: k for k, name in enumerate(head)}
    limit = max_kb_dist * 1000
    nodes, edges = set(), []
    for ln in lines:
        f = ln.split("\t")
        s1, s2 = index[f[0]], index[f[1]]
        assert s1 != s2
        nodes.update((s1, s2))
        dist = f[2].strip()
        if dist.lstrip("+-").lower() in ("inf", "nan") or not int(dist) <= limit:
            continue
        if "maf1" in col and "maf2" in col:
            mafs = [micro(f[col["maf1"]]), micro(f[col["maf2"]])]
            if any(m is None or not m / MICRO >= min_maf for m in mafs):
                continue
        q = micro(f[field - 1])
        if q is None:
            continue
        if abs_value:
            q = abs(q)
        if not q / MICRO >= min_weight:
            continue
        edges.append((s1, s2, q))
    return nodes, edges


def position(label: str) -> int:
    return int(label.rsplit(":", 1)[1])


def clusters(text: str, sites: list[str], min_size: int = 2, **kw) -> tuple[list[int], list[dict]]:
    """(cluster id of every site of `sites` -- the labels of the input, in file order --, table): the table holds one dict per
    cluster of at least min_size sites, in id order, with id, size, first, last, span, edges, sum, mean and density."""
    nodes, edges = tsv_edges(text, sites, **kw)
    parent = {s: s for s in nodes}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b, _ in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    ids = [0] * len(sites)
    rows: dict[int, dict] = {}
    for s in sorted(nodes):       # (increasing site index: a cluster is met first at its smallest site)
        r = find(s)
        if r not in rows:
            rows[r] = dict(id=len(rows) + 1, size=0, first=s, last=s, edges=0, sum=0)
        row = rows[r]
        ids[s] = row["id"]
        row["size"] += 1
        row["last"] = s
    for a, _, q in edges:
        row = rows[find(a)]
        row["edges"] += 1
        row["sum"] += q
    table = []
    for row in rows.values():
        size, n_edges = row["size"], row["edges"]
        row["span"] = position(sites[row["last"]]) - position(sites[row["first"]]) if size > 1 else 0
        row["mean"] = float(Fraction(row["sum"], MICRO * n_edges)) if n_edges else None
        row["density"] = float(Fraction(n_edges, size * (size - 1) // 2)) if size > 1 else None
        if size >= min_size:
            table.append(row)
    return ids, table


def cluster_file(ids: list[int], names: list[str]) -> str:
    """The --cluster_out file: header, then one line per site (names: the first column)."""
    return "site\tcluster\n" + "".join(f"{lab}\t{'NA' if k == 0 else k}\n" for lab, k in zip(names, ids))


def table_file(table: list[dict], names: list[str]) -> str:
    """The --cluster_table file: header, then one line per cluster of the table."""
    rows = [HEADER]
    for r in table:
        rows.append("\t".join([str(r["id"]), str(r["size"]), names[r["first"]], names[r["last"]], str(r["span"]), str(r["edges"]),
                               micro_text(r["sum"]), "NA" if r["mean"] is None else "%.17g" % r["mean"],
                               "NA" if r["density"] is None else "%.17g" % r["density"]]))
    return "\n".join(rows) + "\n"
