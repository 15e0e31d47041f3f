"""LD across chromosomes (ngsld_cross_ld) under every pair-kernel family.

tests/test_gpu_cross.py holds the pass to tests/cross_ref.py on cohorts of 8, 64 and 500 individuals, whose items span 64
candidates.  Here one all-pairs case runs where the pairs come from the other families, on the inputs and cases of
tests/test_gpu_analyses_by_family.py (read there, not changed): 16- and 32-lane groups, the run kernel's last P-form shape, the a/b
run kernel, the multi-wavefront kernel in both forms (with --ignore_miss_data too, and with un-called monomorphic sites) and both
streaming kernels.  The last four are launched item by item, and with pairs_per_item 5 their items are 20 or 5 candidates wide: a
row of 399 candidates is eighty items, no row is a whole number of items, and a wavefront's span of items carries one cell over
many short items.  Each result is held to the rule on that run's own table.

GPU time of this file on one MI355X: see CROSS.md ("What the tests cost")."""
import pytest

import cross_ref
from test_gpu_analyses_by_family import CASES, _input, _new_engine, _tsv
from test_gpu_cross import KNOBS, _bytes, _same

pytestmark = pytest.mark.gpu

KW = dict(ld=("r2", "D"), abs_value=False, linked_min=0.3)


@pytest.mark.parametrize("name", list(CASES))
def test_all_pairs_with_short_items_equal_the_rule_on_own_table(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv("NGSLD_TEST_" + k, raising=False)
    input_name, how, kernel, _, span16 = CASES[name]
    inp = _input(input_name)
    n = len(inp.labels)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        eng.set_tuning(pairs_per_item=5)
        assert eng.plan(ignore_miss_data=inp.masked, extend_out=True) == n * (n - 1) // 2  # (all pairs)
        count = eng.items()["count"]
        if kernel in ("multi", "multi-ab", "stream"):
            assert int(count.max()) == 5 * span16 // 16 < 64
        text = _tsv(eng, inp)
        want = cross_ref.cross(text, inp.labels, 2000, **KW)
        cells, st = eng.cross_ld(inp.labels, 2000, **KW)
        _same(cells, want, KW["ld"])
        assert st["pairs"] == n * (n - 1) // 2 and st["pairs_counted"] == sum(want["n"]) > 0
        assert st["pairs_cross"] == sum(c for c, a, b in zip(want["n"], want["chr1"], want["chr2"]) if a != b) > 0
        if name.endswith("_mono"):
            assert st["pairs_counted"] < st["pairs"]  # (non-finite rows)
        print(f"{name}: items of up to {int(count.max())} candidates, {len(count)} items, {st['cells']} cells, cross_ms {st['cross_ms']:.3f}")
        for env in ({"CROSS_SPAN_ITEMS": "1"}, {"CROSS_SPAN_ITEMS": "3", "RECORD_SLICE_ITEMS": "7", "CROSS_CHUNK_PAIRS": str(st["pairs"] // 10)}):
            for k, v in env.items():
                monkeypatch.setenv("NGSLD_TEST_" + k, v)
            again, _ = eng.cross_ld(inp.labels, 2000, **KW)
            assert _bytes(again) == _bytes(cells), env
    finally:
        eng.close()
