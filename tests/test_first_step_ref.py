"""CPU: the construction of tests/first_step_ref.py, proved against the oracle alone -- what tests/test_gpu_first_step_alone.py
takes for granted is something the reference satisfies by itself: on the disjoint-informative-sets input every pair of sites
from different groups leaves the EM at iteration 0, none of them near the EPSILON tie, and the oracle's four frequencies are
the extended-precision one-step reference to within 64 x 2^-53 (measured: 6.6e-16 at 192 individuals, 6.7e-16 at 257, 1.2e-15
at 500).  Likewise the two special inputs: the reference is finite on every pair of the sanity-fallback input, and NaN with
nIter 0 on exactly one pair of the underflow input."""
import numpy as np
import pytest

import first_step_ref as fr

N_SITES = 60


@pytest.fixture(scope="module", params=[192, 257, 500])
def built(request):
    inp = fr.Input(N_SITES, request.param)
    return inp, inp.o.run()


def test_cross_group_pairs_end_at_iteration_0(built):
    inp, want = built
    assert len(want) == N_SITES * (N_SITES - 1) // 2
    x = inp.cross(want["s1"], want["s2"])
    assert x.sum() == 900
    assert np.all(want["n_iter"][x] == 0)
    assert np.all(want["n_ind_data"] == inp.n_ind)
    assert np.count_nonzero(want["n_iter"][~x] > 1) > 400     # pairs inside a group are ordinary pairs
    assert (inp.o.maf > 0.5).sum() == 20 and np.abs(inp.est_maf - inp.o.maf).max() > 0.05
    assert want["hap"][x][:, 3].min() > 0.01 and want["hap"][x][:, 3].max() > 0.4   # ordinary magnitudes


def test_no_cross_group_pair_near_the_tie(built):
    """eps of iteration 0 = the largest move away from linkage equilibrium at the frequencies handed over."""
    inp, want = built
    x = inp.cross(want["s1"], want["s2"])
    m1, m2 = inp.o.maf[want["s1"][x]], inp.o.maf[want["s2"][x]]
    start = np.stack([(1 - m1) * (1 - m2), (1 - m1) * m2, m1 * (1 - m2), m1 * m2], axis=1)
    eps = np.abs(want["hap"][x] - start).max(axis=1)
    print(f"n_ind {inp.n_ind}: largest eps of a cross-group pair {eps.max():.3e}")
    assert np.all(eps < fr.EPSILON - 1e-9)
    assert eps.max() < 1e-12       # the step moves nothing: not a pair that merely converged early


def test_oracle_is_the_one_step_reference(built):
    inp, want = built
    x = inp.cross(want["s1"], want["s2"])
    dev = fr.deviation(want["hap"][x], inp.step(want["s1"][x], want["s2"][x]))
    print(f"n_ind {inp.n_ind}: oracle - long-double step = {dev:.3e}")
    assert dev <= 64 * fr.ULP


def test_exact_path_agrees_with_long_double():
    """The rational path (used where long double is a double) against the long-double path, on a few pairs."""
    inp = fr.Input(12, 70)
    s1, s2 = np.array([0, 1, 2, 3, 4]), np.array([5, 4, 11, 6, 9])
    a = fr._step_exact(inp.o.gl, inp.o.maf, s1, s2)
    b = fr.one_step(inp.o.gl, inp.o.maf, s1, s2)
    assert float(np.abs(a - b).max()) < 2.0 ** -58


def test_mirror_sites_sit_at_one_half():
    """257 individuals: the two mirror-symmetric sites have their fixed point at 0.5 to the last bit; the two tilted ones are
    handed 0.5 with a dosage sum that is not n (a sum taken under the other labels would be 2n - S: 6e-6 of frequency away).
    With the mirror sites handed 0.5 or a neighbour of it every cross-group pair still ends at iteration 0, away from the tie."""
    inp = fr.Input(N_SITES, 257, mirror=True)
    assert len(inp.half) == 2 and inp.half[0] % 2 != inp.half[1] % 2 and len(inp.tilted) == 2 and inp.tilted[0] % 2 != inp.tilted[1] % 2
    assert np.all(inp.o.maf[inp.half] == 0.5) and np.all(inp.o.maf[inp.tilted] == 0.5)
    off = fr.dosages(inp.o.gl, inp.o.maf)[inp.tilted].sum(axis=1) / (2 * inp.n_ind) - 0.5
    assert np.all((off > 2e-6) & (off < 4e-6))
    for m in (0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0)):
        inp.o.maf[inp.half] = m
        want = inp.o.run()
        x = inp.cross(want["s1"], want["s2"])
        assert x.sum() == 900 and np.all(want["n_iter"][x] == 0)
        m1, m2 = inp.o.maf[want["s1"][x]], inp.o.maf[want["s2"][x]]
        start = np.stack([(1 - m1) * (1 - m2), (1 - m1) * m2, m1 * (1 - m2), m1 * m2], axis=1)
        assert np.abs(want["hap"][x] - start).max() < 4e-6
        assert fr.deviation(want["hap"][x], inp.step(want["s1"][x], want["s2"][x])) <= 64 * fr.ULP


def test_fallback_input_is_finite_in_the_reference():
    o, a, twin = fr.fallback_input(120)
    want = o.run()
    for s in (a, twin):
        p = (want["s1"] == s) | (want["s2"] == s)
        assert p.sum() == 119 and np.all(np.isfinite(want["hap"][p])) and want["n_iter"][p].min() >= 2


def test_underflow_input_is_nan_on_one_pair():
    want = fr.underflow_input().run()
    a, b = fr.UNDERFLOW_SITES
    both = (want["s1"] == a) & (want["s2"] == b)
    assert both.sum() == 1 and np.all(np.isnan(want["hap"][both])) and want["n_iter"][both][0] == 0
    assert np.all(np.isfinite(want["hap"][~both]))
    assert np.count_nonzero((np.isin(want["s1"], (a, b)) | np.isin(want["s2"], (a, b))) & ~both) == 74
