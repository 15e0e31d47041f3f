"""The LD tree (ngsld_ld_tree) under every pair-kernel family.

tests/test_gpu_tree.py holds the pass to tests/tree_ref.py on cohorts of 8, 64 and 500 individuals: the 8-lane group kernels, the
run kernel at 8 slots, the called-genotype kernel -- whose items span 64 candidates.  Here the same comparison runs where the pairs
come from the other families, on the inputs and cases of tests/test_gpu_analyses_by_family.py (read there, not changed): 16- and
32-lane groups, the run kernel's last P-form shape, the a/b run kernel, the multi-wavefront kernel in both forms (with
--ignore_miss_data too, and with un-called monomorphic sites) and both streaming kernels.  Each case runs once as planned and
once with pairs_per_item 5 -- items of 20 or 5 candidates under the last four, shorter than a wavefront --, chunks of a tenth of
the pairs and seven items per launch: the merges keep their bytes, and are held to the rule on that run's own table.

GPU time of this file on one MI355X: see TREE.md ("What the tests cost")."""
import pytest

import tree_ref
from test_gpu_analyses_by_family import CASES, LINKED_KW, _input, _new_engine, _plan, _tsv
from test_gpu_tree import KNOB, PLANT, SLICES, _bytes, _same

pytestmark = pytest.mark.gpu

# the linked pairs' two settings there: absolute r2 at a floor crossed around the 50th candidate (ragged masks, some two thirds of
# the pairs are edges), signed D with a limit inside the window and the maf filter
SETTINGS = [LINKED_KW["abs_r2"], LINKED_KW["signed_D"]]


@pytest.mark.parametrize("name", list(CASES))
def test_tree_equals_the_rule_on_own_table(name, monkeypatch):
    for k in (KNOB, SLICES, PLANT):
        monkeypatch.delenv(k, raising=False)
    input_name, how, kernel, _, span16 = CASES[name]
    inp = _input(input_name)
    eng = _new_engine(inp, how)
    try:
        assert eng.pair_kernel() == kernel
        n0 = _plan(eng, inp)
        assert n0 == len(inp.keys)
        text = _tsv(eng, inp)
        base = []
        for kw in SETTINGS:
            merges, st = eng.ld_tree(**kw)
            nodes, want = tree_ref.tree(text, inp.labels, **kw)
            _same(merges, want)
            assert st["chunks"] == 1 and st["nodes"] == len(nodes) and st["merges"] == len(want) > 50
            base.append(merges)
        # short items, small chunks, seven items a launch
        eng.set_tuning(pairs_per_item=5)
        assert _plan(eng, inp) == n0
        count = eng.items()["count"]
        assert int(count.sum()) == n0
        if kernel in ("multi", "multi-ab", "stream"):  # (launched item by item: the run families' items span 64 candidates)
            assert int(count.max()) == 5 * span16 // 16 < 64
        monkeypatch.setenv(KNOB, str(n0 // 10))
        monkeypatch.setenv(SLICES, "7")
        for kw, was in zip(SETTINGS, base):
            merges, st = eng.ld_tree(**kw)
            assert _bytes(merges) == _bytes(was), kw
            assert st["chunks"] > 5
        print(f"{name}: {n0} pairs, merges {[len(m['q']) for m in base]}, the last run in {st['chunks']} chunks, {st['rounds']} rounds, "
              f"{st['displaced']} forest edges displaced")
    finally:
        eng.close()
