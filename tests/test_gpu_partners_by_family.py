"""LD partners (ngsld_partners) under every pair-kernel family.

tests/test_gpu_partners.py holds the pass, byte for byte, to tests/partners_ref.py on cohorts of 8, 64 and 500 individuals: the
8-lane group kernels, the run kernel at 8 slots, the called-genotype kernel -- whose items span 64 candidates.  Here the same
comparison runs where the pairs come from the other families, on the inputs, cases and cuts of
tests/test_gpu_analyses_by_family.py (read there, not changed): 16- and 32-lane groups, the run kernel's last P-form shape, the
a/b run kernel, the multi-wavefront kernel in both forms (with --ignore_miss_data too, and with un-called monomorphic sites) and
both streaming kernels.  The last four are launched item by item, and with pairs_per_item 5 their items are 20 or 5 candidates
wide: no row is a whole number of items, every item is shorter than a wavefront, and a site's row end arrives in many small
hand-overs.  Each result is held to the rule on that run's own table (Engine.run + run_text).

GPU time of this file on one MI355X: see PARTNERS.md ("What the tests cost")."""
import math

import numpy as np
import pytest

from test_gpu_analyses_by_family import CASES, LINKED_KW, _input, _new_engine, _plan
from test_gpu_linked import Table
from test_gpu_partners import KNOBS, _check, _want

pytestmark = pytest.mark.gpu

# the linked pairs' two settings there: absolute r2 at a floor crossed around the 50th candidate (most sites have more than 5
# partner rows, the masks are ragged), signed D with a limit inside the window and the maf filter
SETTINGS = [(5, LINKED_KW["abs_r2"]), (64, LINKED_KW["abs_r2"]), (5, LINKED_KW["signed_D"])]


def _all(eng, tab):
    out = {}
    for k, kw in SETTINGS:
        res, st = _check(eng, tab, k, **kw)
        out[(k, kw["field"])] = ({a: res[a].tobytes() for a in ("rows", "partner", "value_micro")}, st)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_partners_equal_the_rule_on_own_table(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    input_name, how, kernel, _, _ = CASES[name]
    inp = _input(input_name)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        assert _plan(eng, inp) == len(inp.keys)
        tab = Table(eng, inp.labels)
        assert [(int(a), int(b)) for a, b in zip(tab.s1, tab.s2)] == inp.keys
        got = _all(eng, tab)
        rows = _want(tab, eng.n_sites, None, **LINKED_KW["abs_r2"])[0]
        print(f"{name}: partner rows a site at the r2 floor: max {int(rows.max())} min {int(rows.min())}")
        assert (rows > 5).any() and all(st["chunks"] == 1 for _, st in got.values())  # (lists that are cut)
        if name.endswith("_mono"):
            # un-called monomorphic sites: non-finite rows, never partner rows whatever the floor; the replayed pairs carry their
            # replayed digits
            for f in (6, 7):
                col = [ln.split("\t")[f - 1] for ln in tab.rows]
                bad = sum(1 for v in col if "nan" in v or "inf" in v)
                assert bad > 0
                _, st = _check(eng, tab, 5, field=f, min_weight=-math.inf, abs_value=False)
                assert st["rows_counted"] == len(tab.rows) - bad
            info = eng.replay_info()
            assert info["pairs_flagged"] > 0 and info["pairs_on_device"] > 0
    finally:
        eng.close()


CUTS = {
    # name: (case, pairs per item, environment)
    "multi_items5": ("multi", 5, {}),
    "multi-ab_items5_chunks": ("multi-ab", 5, {"NGSLD_TEST_PARTNERS_CHUNK_PAIRS": "tenth"}),
    "stream_items5_slices7": ("stream_resident", 5, {"NGSLD_TEST_PARTNERS_CHUNK_PAIRS": "tenth", "NGSLD_TEST_RECORD_SLICE_ITEMS": "7"}),
}


@pytest.mark.parametrize("cut", list(CUTS))
def test_cut_small_gives_the_same_bytes(cut, monkeypatch):
    """pairs_per_item 5: items of 20 candidates under the multi-wavefront kernel and of 5 under the streaming kernel; chunks of a
    tenth of the pairs; seven items per launch.  The lists keep their bytes and are held to the rule again."""
    name, ppi, env = CUTS[cut]
    input_name, how, kernel, _, span16 = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    inp = _input(input_name)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        n0 = _plan(eng, inp)
        tab = Table(eng, inp.labels)
        base = _all(eng, tab)
        eng.set_tuning(pairs_per_item=ppi)
        assert _plan(eng, inp) == n0 == len(inp.keys)
        count = eng.items()["count"]
        span = ppi * span16 // 16
        assert int(count.max()) == span < 64 and int(count.sum()) == n0
        for k, v in env.items():
            monkeypatch.setenv(k, str(n0 // 10) if v == "tenth" else v)
        got = _all(eng, tab)
        for key, (as_bytes, st) in got.items():
            assert as_bytes == base[key][0], (cut, key)
            assert (st["chunks"] > 5) if "NGSLD_TEST_PARTNERS_CHUNK_PAIRS" in env else (st["chunks"] == 1)
    finally:
        eng.close()
