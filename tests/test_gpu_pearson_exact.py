"""GPU: r2_ExpG bit for bit, in every pair-kernel family, on inputs whose Pearson moment is exact (tests/pearson_ref.py).

check_records holds r2_ExpG to 1e-9 and tests/test_gpu_pair_moments.py compares pass-on with pass-off to 1e-9: a moment wrong
in the 11th digit -- a padding individual leaking in, a K chunk mis-indexed for one half-tile, a partial sum kept in a narrower
type, a tile element mapped to a neighbouring record of nearly equal value -- passes both.  On exact_sites' inputs the moment has
no rounding in any summation order, centred or not, fused or not, on the vector or the matrix pipe, so every family must give
predict_r2's bits on every pair, finite or NaN: group (8 / 16 / 32 lanes), run (3 to 10 slots, with pair_ld_moments_kernel in
front and with NGSLD_TEST_PAIR_MOMENTS=0 -- hence the same bits pass-on and pass-off), ab, multi, multi-ab, both streaming
kernels, the called-genotype kernel, and the masked kernels under --ignore_miss_data.  The replay is off (Engine.set_replay(False):
every record is the kernels' own value).

The pass's map from tile element to record (128 x 64 tiles, the items' masks) is walked at 300 sites x 500 individuals: rows
127..129 straddle a row block and candidates 64 / 65 a tile; a banded plan whose row ends fall inside tiles; masks with holes
(min_maf, rnd_sample); launches cut at 3,000 pairs, grids of 7 workgroups, batches of 700 pairs.  There the prediction itself
shows that neighbouring records differ in bits, so a shifted map cannot hide.  The families launched item by item run with
pairs_per_item 5 as well.  (At 64 sites every row's last candidate is site 63, a constant one: row ends are the 300-site cuts'.)  (S12, the first step's dosage sum, is not exact on these inputs -- num / den rounds -- and stays with
tests/test_gpu_pair_moments.py and tests/test_gpu_first_step.py.)

GPU time of this file on one MI355X: see README.md (the tests row)."""
import contextlib
import functools

import numpy as np
import pytest

from ngsld_amd import capi, shard, synth
from oracle import orc
from pearson_ref import adjacent_differ, exact_called_sites, exact_sites, predict_r2
from test_gpu_pair_moments import _env
from util import same_bits

pytestmark = pytest.mark.gpu

N_SITES = 64
MAP_SITES, MAP_IND = 300, 500


@contextlib.contextmanager
def _engine(how=None, **env):
    """A context of its own, the replay off; how: NGSLD_PAIR_KERNEL, read when the context is made (env likewise)."""
    with _env(NGSLD_PAIR_KERNEL=how, **env):
        eng = capi.Engine(0)
    try:
        eng.set_replay(False)
        yield eng
    finally:
        eng.close()


@functools.lru_cache(maxsize=2)
def _sites(n_sites, n_ind, missing=0):
    return exact_sites(n_sites, n_ind, 7000 + n_ind + missing, missing=missing)


def _all_pairs(n_sites):
    return tuple(x.astype(np.uint64) for x in np.triu_indices(n_sites, 1))


def _hold(eng, E, kernel, load, keys, moments=None, pd=None, masked=False, run_env=None, ppi=0, **plan):
    """Load, plan and run; the plan's pairs are `keys` and every r2_ExpG is the prediction's bits."""
    load(eng)
    assert eng.pair_kernel() == kernel
    eng.set_pos_dist(pd)
    if ppi:
        eng.set_tuning(pairs_per_item=ppi)
    n = eng.plan(extend_out=True, ignore_miss_data=masked, **plan)
    knobs = dict(run_env or {})
    if moments is not None:
        knobs["NGSLD_TEST_PAIR_MOMENTS"] = "1" if moments else "0"
    with _env(**knobs):
        s1, s2, std, _ = eng.run()
    assert n == len(s1) == len(keys[0]) and np.array_equal(s1, keys[0]) and np.array_equal(s2, keys[1])
    want = predict_r2(E, eng.maf(), s1, s2)
    _same(std["r2_ExpG"], want, s1, s2)
    return want


def _same(got, want, s1, s2):
    ok = same_bits(got, want)
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, (f"r2_ExpG differs in bits on {len(bad)} of {len(ok)} pairs; first (s1, s2, got, want): "
                           f"{[(int(s1[k]), int(s2[k]), float(got[k]).hex(), float(want[k]).hex()) for k in bad[:4]]}")


# (n_ind, NGSLD_PAIR_KERNEL, pair_kernel(), the pass on / off or None where there is none): the dispatch of pair_config and the
# cohorts of tests/test_gpu_analyses_by_family.py, and the other families the override gives a shape at a cohort
CASES = [
    (61, None, "group", None),      # 8-lane groups, three padding individuals
    (100, None, "group", None),     # 16-lane groups
    (160, None, "group", None),     # 32-lane groups
    (192, None, "run", True), (192, None, "run", False),    # three full slots
    (257, None, "run", True), (257, None, "run", False),    # one individual in slot 5
    (500, None, "run", True), (500, None, "run", False),    # eight slots
    (576, None, "run", True), (576, None, "run", False),    # nine slots: the DOSE = false instantiation of the pass
    (640, None, "run", True), (640, None, "run", False),    # ten
    (640, "ab", "ab", None),
    (700, None, "ab", None),
    (700, "multi", "multi", None),  # 2 x 6
    (1000, None, "multi", None),    # 2 x 8
    (1500, None, "multi-ab", None),  # 2 x 12
    (1500, "multi", "multi", None),  # 4 x 6
    (5121, None, "multi-ab", None),  # 8 x 11
    (5121, "bres", "stream", None),
    (5121, "stream", "stream", None),
]


def _id(case):
    n_ind, how, kernel, moments = case
    return f"{n_ind}-{kernel}" + (f"-asked_{how}" if how else "") + ("" if moments is None else ("-pass_on" if moments else "-pass_off"))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_family_gives_the_exact_bits(case):
    n_ind, how, kernel, moments = case
    gl, E, _ = _sites(N_SITES, n_ind)
    with _engine(how) as eng:
        want = _hold(eng, E, kernel, lambda e: e.set_geno_raw(gl), _all_pairs(N_SITES), moments=moments)
    assert 0.7 < np.isfinite(want).mean() < 0.8  # (the scale-1 sites are constant: NaN on all their pairs, in the records too)


@pytest.mark.parametrize("moments", [True, False], ids=["pass_on", "pass_off"])
def test_run_kernel_through_set_geno_lkl(moments):
    """The same triples handed over normalised, with the oracle's frequencies."""
    gl, E, _ = _sites(N_SITES, 500)
    o = orc.Oracle(gl, n_threads=4)
    with _engine() as eng:
        _hold(eng, E, "run", lambda e: e.set_geno_lkl(gl, o.maf), _all_pairs(N_SITES), moments=moments)
        assert np.array_equal(eng.maf(), o.maf)


def test_called_genotype_kernel():
    raw, E, _ = exact_called_sites(N_SITES, 250, 7250)
    with _engine() as eng:
        want = _hold(eng, E, "hard", lambda e: e.set_geno_raw(raw), _all_pairs(N_SITES))
    assert np.isfinite(want).all()


@pytest.mark.parametrize("n_ind,how,kernel", [(500, None, "run"), (1500, None, "multi-ab"), (5121, None, "multi-ab"),
                                              (5121, "bres", "stream"), (5121, "stream", "stream")],
                         ids=lambda v: "auto" if v is None else str(v))
def test_masked_kernels_give_the_exact_bits(n_ind, how, kernel):
    """--ignore_miss_data with a tenth of the individuals without data at every site: pearson_r runs over ALL individuals
    (ngsLD.cpp:290), an individual without data at e = 1.0.  500: the masked run kernel, no pass in front of it."""
    gl, E, _ = _sites(N_SITES, n_ind, n_ind // 10)
    with _engine(how) as eng:
        want = _hold(eng, E, kernel, lambda e: e.set_geno_raw(gl, ignore_miss_data=True), _all_pairs(N_SITES), masked=True)
    assert np.isfinite(want).all()


@pytest.mark.parametrize("n_ind,how,kernel", [(1000, None, "multi"), (1500, None, "multi-ab"), (5121, "bres", "stream"),
                                              (5121, "stream", "stream")], ids=lambda v: "auto" if v is None else str(v))
def test_item_by_item_families_with_short_items(n_ind, how, kernel):
    """pairs_per_item 5: items of 20 or 5 candidates, no row a whole number of them -- the record of a pair is found through
    its item's mask and first_record."""
    gl, E, _ = _sites(N_SITES, n_ind)
    with _engine(how) as eng:
        _hold(eng, E, kernel, lambda e: e.set_geno_raw(gl), _all_pairs(N_SITES), ppi=5)
        assert int(eng.items()["count"].max()) in (5, 20)


# ---- the pass's map from tile element to record: 300 sites x 500 individuals ----
@functools.lru_cache(maxsize=1)
def _map_input():
    gl, E, c = exact_sites(MAP_SITES, MAP_IND, 7300)
    chrs, pos = synth.make_positions(MAP_SITES, 7300, max_gap=200)
    return gl, E, c, shard.pos_dist_from_positions(chrs, pos), orc.Oracle(gl, n_threads=4).maf


def _oracle_keys(gl, pd=None, **kw):
    """The plan's pairs as the oracle enumerates them (its window, its maf filter, its sub-sampling)."""
    rec = orc.Oracle(gl, pos_dist=pd, n_threads=16, **kw).run()
    return rec["s1"].astype(np.uint64), rec["s2"].astype(np.uint64)


MAP_CUTS = ["one_launch", "banded", "min_maf", "rnd_sample", "launches_of_3000_pairs", "grids_of_7_workgroups", "batches_of_700_pairs"]


@pytest.mark.parametrize("cut", MAP_CUTS)
def test_tile_to_record_map_of_the_pass(cut):
    gl, E, c, pd, maf = _map_input()
    plan, run_env, make_env, use_pd = {}, {}, {}, None
    keys = _all_pairs(MAP_SITES)
    if cut == "banded":  # some 100 candidates a row: row ends inside tiles, the row blocks' last tiles beyond the band
        use_pd, plan = pd, dict(max_kb_dist=10)
        keys = _oracle_keys(gl, pd, max_kb_dist=10)
        per_row = np.bincount(keys[0].astype(np.int64), minlength=MAP_SITES)
        assert 64 < per_row[:150].min() and per_row.max() < 192 and len(keys[0]) < 40_000
    elif cut == "min_maf":
        # at the median of the oracle's frequencies: the masks have holes.  A site's frequency is half its centre -- on the device
        # exactly: est_maf's sums are n c and 2 n (held below) -- and the median is the oracle's value of one of the 76 sites at
        # 0.375, a last bit beside it or not.  With the replay off the tie is the device's to settle (ngsLD.cpp:270 on its own
        # frequencies), so the pairs are enumerated by that rule here, not taken from the oracle: whole blocks of eight sites drop
        # out of every item they lie in
        plan = dict(min_maf=float(np.median(maf)))
        assert abs(plan["min_maf"] - 0.375) < 1e-12
        kept = c / 2 >= plan["min_maf"]
        assert 140 <= kept.sum() <= 220
        keys = tuple(x[kept[keys[0].astype(np.int64)] & kept[keys[1].astype(np.int64)]] for x in keys)
    elif cut == "rnd_sample":
        plan = dict(rnd_sample=0.3, seed=11)
        keys = _oracle_keys(gl, **plan)
        assert 10_000 < len(keys[0]) < 17_000
    elif cut == "launches_of_3000_pairs":
        run_env = {"NGSLD_TEST_MOMENTS_PAIRS": "3000"}
    elif cut == "grids_of_7_workgroups":
        run_env = {"NGSLD_TEST_MAX_BLOCKS": "7"}
    elif cut == "batches_of_700_pairs":
        make_env = {"NGSLD_TEST_BATCH_PAIRS": "700"}
    # a map that is off by a record, a candidate or a row would show: neighbouring records differ in bits
    share = adjacent_differ(predict_r2(E, maf, *keys))
    print(f"{cut}: {len(keys[0])} pairs, neighbouring records differ in bits on {share:.4f} of those with a finite value")
    assert share > 0.99
    with _engine(**make_env) as eng:
        _hold(eng, E, "run", lambda e: e.set_geno_raw(gl), keys, moments=True, pd=use_pd, run_env=run_env, **plan)
        assert np.array_equal(eng.maf(), c / 2)
        if cut == "one_launch":  # ... and as ONE launch for certain: the records left on the device by ngsld_run_device
            import torch
            n = len(keys[0])
            dev = torch.device("cuda", 0)
            d_std = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
            d_ext = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
            with _env(NGSLD_TEST_PAIR_MOMENTS="1"):
                eng.run_device(0, MAP_SITES, d_std.data_ptr(), d_ext.data_ptr(), None)
                torch.cuda.synchronize()
            std = d_std.cpu().numpy().view(capi.REC_STD)
            _same(std["r2_ExpG"], predict_r2(E, eng.maf(), *keys), *keys)
