"""GPU: the error write_pair's text margin of r2_ExpG has to cover, in every pair-kernel family.

write_pair (ld_em.h) flags a pair whose r2_ExpG lies within 32 ulp * (k / (std1 std2) + 0.5) of a sixth-decimal rounding point
-- k = 6 where pair_ld_moments_kernel supplied the moment, k = 2 elsewhere -- and the replay then prints the reference's digits.
That holds the text to the reference byte for byte only if no kernel is ever further from the reference than its margin: a larger
distance is a wrong printed digit waiting to happen, and neither the 1e-9 bar of check_records (the margin is about 2e-13 on
ordinary inputs) nor the text tests (an error of 1e-11 moves a digit on 2 pairs in 10^5) would see it.  So here the distance
itself is held to the margin, on real-valued raw input whose expected genotypes have a graded spread (pearson_ref.graded_sites:
1 / (std1 std2) in every octave from 2^4 to kPearsonCond = 2^13, beyond which a pair is replayed whatever its value), against
the oracle's long-double recurrence (within 2e-5 of the margin of a two-pass long-double evaluation: tests/test_pearson_ref.py),
with the replay off.  The bar is 1, the margin as it stands; the ratios reached are printed per octave and recorded in DESIGN.md
(section 4.2).  The called-genotype kernel takes no real-valued input: its moment is held bit for bit in
tests/test_gpu_pearson_exact.py.

GPU time of this file on one MI355X: see README.md (the tests row)."""
import functools

import numpy as np
import pytest

from oracle import orc
from pearson_ref import PEARSON_COND, graded_sites, pair_cond, text_margin
from test_gpu_pair_moments import _env
from test_gpu_pearson_exact import _engine

pytestmark = pytest.mark.gpu

N_SITES = 96
# name: (n_ind, NGSLD_PAIR_KERNEL, pair_kernel(), the pass on / off or None where there is none): a case per family of
# tests/test_gpu_pearson_exact.py
CASES = {
    "group8": (61, None, "group", None),
    "group16": (100, None, "group", None),
    "group32": (160, None, "group", None),
    "run5_pass_on": (257, None, "run", True),
    "run5_pass_off": (257, None, "run", False),
    "run8_pass_on": (500, None, "run", True),
    "run8_pass_off": (500, None, "run", False),
    "run10_pass_on": (640, None, "run", True),
    "run10_pass_off": (640, None, "run", False),
    "ab": (700, None, "ab", None),
    "multi": (1000, None, "multi", None),
    "multi-ab": (1500, None, "multi-ab", None),
    "multi-ab_8x11": (5121, None, "multi-ab", None),
    "stream_resident": (5121, "bres", "stream", None),
    "stream_plain": (5121, "stream", "stream", None),
}


@functools.lru_cache(maxsize=2)
def _reference(n_ind):
    """(raw, the oracle's records, 1 / (std1 std2) of every pair from the oracle's expected genotypes): once per cohort."""
    raw = graded_sites(N_SITES, n_ind, 8000 + n_ind)
    o = orc.Oracle(raw, n_threads=16)
    want = o.run()
    assert len(want) == N_SITES * (N_SITES - 1) // 2
    return raw, want, pair_cond(o.expg, want["s1"], want["s2"])


@pytest.mark.parametrize("name", list(CASES))
def test_distance_from_the_reference_is_inside_the_text_margin(name):
    n_ind, how, kernel, moments = CASES[name]
    raw, want, cond = _reference(n_ind)
    with _engine(how) as eng:
        eng.set_geno_raw(raw)
        assert eng.pair_kernel() == kernel
        eng.set_pos_dist(None)
        assert eng.plan(extend_out=True) == len(want)
        with _env(NGSLD_TEST_PAIR_MOMENTS=None if moments is None else ("1" if moments else "0")):
            s1, s2, std, _ = eng.run()
    assert np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
    held = np.isfinite(cond) & (cond <= PEARSON_COND)
    octave = np.floor(np.log2(cond))
    assert held.mean() >= 0.60 and all(np.count_nonzero(held & (octave == k)) >= 50 for k in range(4, 13))
    got, ref = std["r2_ExpG"][held], want["r2pear"][held]
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    ratio = np.abs(got - ref) / text_margin(cond[held], from_pass=bool(moments))
    per_octave = " ".join(f"2^{k}:{ratio[octave[held] == k].max():.2e}" for k in range(4, 13))
    print(f"{name} ({kernel}, {n_ind} individuals, k = {6 if moments else 2}): largest |r2_ExpG - reference| / margin = {ratio.max():.3e} "
          f"over {held.sum()} pairs; per octave of 1 / (std1 std2): {per_octave}")
    worst = int(np.argmax(ratio))
    assert ratio.max() <= 1.0, (f"{name}: {np.count_nonzero(ratio > 1)} pairs further from the reference than the text margin; worst "
                                f"{ratio.max():.3e} at pair ({int(s1[held][worst])}, {int(s2[held][worst])}), 1 / (std1 std2) = {cond[held][worst]:.1f}")
