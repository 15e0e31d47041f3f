"""tests/cluster_ref.py -- the restatement of CLUSTERS.md that the GPU tests compare ngsld_clusters with -- held to tables worked
by hand.  No GPU."""
import math

import cluster_ref

SITES = ["1:100", "1:200", "1:300", "1:400", "1:500", "1:600", "1:700", "2:50", "2:150", "2:900"]
A, B, C_, D, E, F, G, H, I, Z = range(10)


def _row(s1, s2, dist, r2="0.000000", d="0.000000", dp="0.000000", r2e="0.000000", maf=None):
    cells = [SITES[s1], SITES[s2], str(dist), r2e, d, dp, r2]
    if maf is not None:
        cells += ["10", maf[0], maf[1]] + ["0.250000"] * 4 + ["0.100000", "0.100000", "1.000000", "-10.000000", "5"]
    return "\t".join(cells)


# a chain a-b-c (b-c exactly at the floor), a triangle d-e-f, g one millionth below the floor, NaN and inf values, a pair
# across chromosomes; the site 2:900 is in no row
TABLE = "\n".join([
    _row(A, B, 100, "0.900000"),
    _row(A, C_, 200, "0.100000"),
    _row(B, C_, 100, "0.500000"),
    _row(C_, D, 100, "nan"),
    _row(D, E, 100, "0.800000"),
    _row(D, F, 200, "0.600000"),
    _row(E, F, 100, "0.700000"),
    _row(F, G, 100, "0.499999"),
    _row(G, H, "inf", "0.990000"),
    _row(H, I, 100, "inf"),
]) + "\n"


def test_chain_triangle_singletons_and_a_site_in_no_row():
    ids, table = cluster_ref.clusters(TABLE, SITES, min_size=1)
    assert ids == [1, 1, 1, 2, 2, 2, 3, 4, 5, 0]
    assert [r["id"] for r in table] == [1, 2, 3, 4, 5]
    chain, tri = table[0], table[1]
    assert chain == dict(id=1, size=3, first=A, last=C_, span=200, edges=2, sum=1_400_000, mean=0.7, density=2 / 3)
    assert tri == dict(id=2, size=3, first=D, last=F, span=200, edges=3, sum=2_100_000, mean=0.7, density=1.0)
    for r, s in zip(table[2:], (G, H, I)):
        assert r == dict(id=r["id"], size=1, first=s, last=s, span=0, edges=0, sum=0, mean=None, density=None)


def test_a_value_exactly_min_weight_is_an_edge_and_one_millionth_below_is_not():
    nodes, edges = cluster_ref.tsv_edges(TABLE, SITES)
    assert (B, C_, 500_000) in edges and not any(e[:2] == (F, G) for e in edges)
    assert nodes == set(range(9))
    ids, _ = cluster_ref.clusters(TABLE, SITES, min_weight=0.499999)
    assert ids == [1, 1, 1, 2, 2, 2, 2, 3, 4, 0]          # (g joins the triangle)
    ids, _ = cluster_ref.clusters(TABLE, SITES, min_weight=0.500001)
    assert ids == [1, 1, 2, 3, 3, 3, 4, 5, 6, 0]          # (c leaves the chain)


def test_nan_inf_and_a_dist_across_chromosomes_are_never_edges():
    _, edges = cluster_ref.tsv_edges(TABLE, SITES, min_weight=-math.inf)
    pairs = {e[:2] for e in edges}
    assert (C_, D) not in pairs and (H, I) not in pairs and (G, H) not in pairs
    assert pairs == {(A, B), (A, C_), (B, C_), (D, E), (D, F), (E, F), (F, G)}


def test_min_size_filters_the_table_and_not_the_ids():
    ids1, t1 = cluster_ref.clusters(TABLE, SITES, min_size=1)
    ids2, t2 = cluster_ref.clusters(TABLE, SITES)
    ids4, t4 = cluster_ref.clusters(TABLE, SITES, min_size=4)
    assert ids1 == ids2 == ids4
    assert [r["id"] for r in t2] == [1, 2] and t4 == [] and len(t1) == 5


def test_absolute_against_signed_values():
    text = "\n".join([_row(A, B, 100, d="-0.600000"), _row(B, C_, 100, d="0.600000"), _row(C_, D, 100, d="-0.100000")]) + "\n"
    ids, table = cluster_ref.clusters(text, SITES, field=5)
    assert ids[:4] == [1, 1, 1, 2] and table[0]["sum"] == 1_200_000 and table[0]["mean"] == 0.6
    ids, table = cluster_ref.clusters(text, SITES, field=5, abs_value=False)
    assert ids[:4] == [1, 2, 2, 3] and table[0]["id"] == 2 and table[0]["sum"] == 600_000
    ids, table = cluster_ref.clusters(text, SITES, field=5, abs_value=False, min_weight=-0.6)
    assert ids[:4] == [1, 1, 1, 1]                           # (-0.6 >= -0.6: the floor itself, signed)
    assert table[0]["sum"] == -100_000 and table[0]["mean"] == float.fromhex("-0x1.1111111111111p-5")  # -0.1 / 3
    assert table[0]["density"] == 0.5


def test_ids_follow_the_smallest_site_not_the_order_of_the_rows():
    text = "\n".join([_row(E, F, 100, "0.900000"), _row(C_, D, 100, "0.900000"), _row(B, G, 500, "0.900000"),
                      _row(A, F, 500, "0.900000"), _row(B, C_, 100, "0.100000")]) + "\n"
    ids, table = cluster_ref.clusters(text, SITES)
    assert ids == [1, 2, 3, 3, 1, 1, 2, 0, 0, 0]
    assert [(r["id"], r["first"], r["last"], r["span"], r["size"]) for r in table] == [(1, A, F, 500, 3), (2, B, G, 500, 2), (3, C_, D, 100, 2)]
    assert table[1]["density"] == 1.0 and table[0]["density"] == 2 / 3


def test_distance_limit_is_not_strict_and_the_maf_filter_reads_the_printed_maf():
    ids, _ = cluster_ref.clusters(TABLE, SITES, max_kb_dist=0.1)
    assert ids == [1, 1, 1, 2, 2, 2, 3, 4, 5, 0]          # (dist 100 <= 100; d-f at 200 is out, d-e-f holds by its other edges)
    ids, table = cluster_ref.clusters(TABLE, SITES, max_kb_dist=0.0999)
    assert ids == [1, 2, 3, 4, 5, 6, 7, 8, 9, 0] and table == []
    ext = "\n".join([_row(A, B, 100, "0.900000", maf=("0.050000", "0.300000")), _row(B, C_, 100, "0.900000", maf=("0.300000", "0.049999")),
                     _row(C_, D, 100, "0.900000", maf=("0.300000", "nan")), _row(D, E, 100, "0.900000", maf=("nan", "0.300000"))]) + "\n"
    assert cluster_ref.clusters(ext, SITES, min_maf=0.05)[0][:5] == [1, 1, 2, 3, 4]
    assert cluster_ref.clusters(ext, SITES)[0][:5] == [1, 1, 1, 2, 3]      # (a NaN maf never passes, even at 0)
    head = "\t".join(cluster_ref.COLUMNS) + "\n"
    assert cluster_ref.clusters(head + ext, SITES, min_maf=0.05) == cluster_ref.clusters(ext, SITES, min_maf=0.05)


def test_the_two_files():
    ids, table = cluster_ref.clusters(TABLE, SITES)
    assert cluster_ref.cluster_file(ids, SITES).splitlines()[:3] == ["site\tcluster", "1:100\t1", "1:200\t1"]
    assert cluster_ref.cluster_file(ids, SITES).endswith("2:150\t5\n2:900\tNA\n")
    assert cluster_ref.table_file(table, SITES) == (
        "cluster\tsize\tfirst\tlast\tspan\tedges\tsum\tmean\tdensity\n"
        "1\t3\t1:100\t1:300\t200\t2\t1.400000\t0.69999999999999996\t0.66666666666666663\n"
        "2\t3\t1:400\t1:600\t200\t3\t2.100000\t0.69999999999999996\t1\n")
    _, t1 = cluster_ref.clusters(TABLE, SITES, min_size=1)
    assert cluster_ref.table_file(t1, SITES).splitlines()[3] == "3\t1\t1:700\t1:700\t0\t0\t0.000000\tNA\tNA"
