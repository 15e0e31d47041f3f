"""GPU: the run kernel's first EM step from the sites' posterior dosages (ld_kernel_run.h, site_dose_kernel in ld_prep.hip)
against the oracle, and against the same kernel with the step switched off (NGSLD_TEST_FIRST_STEP=0: every pair starts at
iteration 0 with the per-individual step, as before the step existed).

Every pair starts at linkage equilibrium, where iteration 0 is S12 = sum d1 d2 and two per-site sums.  What can go wrong there
and is held here, at the smallest shapes that reach it (some 45,000 pairs each): padding lanes and the slot counts (the
reciprocal shared by a lane's slots, a padding lane's den), sites whose alleles the kernel relabels, pairs that leave the EM at
iteration 0 or 1 (the given step's bookkeeping is then all there is), sites that may not take part (not dose_ok) beside sites
that do, and the knob itself at the headline's shape.  Bars: tests/util.py -- nIter and sample_size exact, values to 1e-9,
degenerate pairs bit for bit.

The seeds of test_pairs_that_leave_at_iteration_0_or_1 were chosen on the CPU with the oracle."""
import contextlib
import os

import numpy as np
import pytest

from ngsld_amd import capi, shard, synth
from oracle import orc
from util import TOL, check_records, close, same_bits

pytestmark = pytest.mark.gpu

VALUES = (("hap", "ext"), ("D", "std"), ("Dp", "std"), ("r2", "std"), ("r2_ExpG", "std"))


@contextlib.contextmanager
def _first_step(on: bool):
    """The knob is read when a matrix is set."""
    old = os.environ.get("NGSLD_TEST_FIRST_STEP")
    os.environ["NGSLD_TEST_FIRST_STEP"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["NGSLD_TEST_FIRST_STEP"]
        else:
            os.environ["NGSLD_TEST_FIRST_STEP"] = old


def _run(eng, load, pd, on, kernel="run", **plan):
    with _first_step(on):
        load(eng)
    assert eng.pair_kernel() == kernel
    eng.set_pos_dist(pd)
    n = eng.plan(extend_out=True, **plan)
    s1, s2, std, ext = eng.run()
    assert len(s1) == n
    return s1, s2, std, ext


def _differ(a, b):
    """Pairs on which two runs' haplotype frequencies are not the same bits."""
    return ~np.all(same_bits(a[3]["hap"], b[3]["hap"]), axis=1)


def _against_oracle(engine, raw, o=None, kernel="run"):
    """All pairs with the step on, held to the oracle; the step off must give the same nIter on every pair -- and the step
    must have been taken: it moves last bits somewhere (another kernel family has no such step: the same bits everywhere)."""
    o = o or orc.Oracle(raw, n_threads=16)
    want = o.run()
    on = _run(engine, lambda e: e.set_geno_raw(raw), None, True, kernel)
    assert np.array_equal(on[0], want["s1"]) and np.array_equal(on[1], want["s2"])
    check_records(on[2], on[3], want)
    off = _run(engine, lambda e: e.set_geno_raw(raw), None, False, kernel)
    check_records(off[2], off[3], want)
    assert np.array_equal(on[3]["n_iter"], off[3]["n_iter"])
    if kernel == "run":
        assert _differ(on, off).any(), "the first step from dosages was not taken on any pair"
    else:
        assert not _differ(on, off).any()
    return want, o


@pytest.mark.parametrize("n_ind", [500, 192, 257, 129])
def test_padding_and_slot_counts(engine, n_ind):
    """500: eight slots, 12 padding lanes in the last; 192: three full slots, no padding; 257: one individual in the last of five
    slots.  129 -- one individual in the last of three -- is the lockstep (group) kernel's by cohort size (five 32-lane slots,
    pair_config): it has no such step, the knob switches nothing there, and the records are the oracle's all the same."""
    want, _ = _against_oracle(engine, synth.make_gl_numpy(300, n_ind, 1100 + n_ind, depth=6.0), kernel="group" if n_ind == 129 else "run")
    assert len(want) == 300 * 299 // 2


def test_relabelled_sites(engine):
    """Every other site's alleles trade places: its frequency lies in (0.5, 0.95) and the kernel relabels it.  Pairs with
    neither, the first, the second and both sites relabelled all occur."""
    raw = synth.make_gl_numpy(300, 500, 1201, depth=6.0)
    raw[1::2] = raw[1::2, :, ::-1].copy()
    want, o = _against_oracle(engine, raw)
    hi = o.maf > 0.5
    assert np.all((o.maf[1::2] > 0.5) & (o.maf[1::2] < 0.95)) and 100 < hi.sum() < 200
    kinds = set(zip(hi[want["s1"]].tolist(), hi[want["s2"]].tolist()))
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


def _with_rare_sites(n_sites, n_ind, seed, n_rare=40):
    """SNP-called sites among which n_rare hold one to three heterozygous carriers, called without doubt: pairs of two such
    sites have |D| below EPSILON (the EM leaves at iteration 0), pairs with an ordinary site leave a step or two later."""
    raw = synth.make_gl_numpy(n_sites, n_ind, seed, depth=8.0)
    rng = np.random.default_rng([seed, 77])
    for s in rng.choice(n_sites, n_rare, replace=False):
        k = int(rng.integers(1, 4))
        raw[s] = (1.0, 1e-9, 1e-30)
        raw[s, rng.choice(n_ind, k, replace=False)] = (1e-9, 1.0, 1e-9)
    return raw


def test_pairs_that_leave_at_iteration_0_or_1(engine):
    """The oracle has 103 pairs with nIter 0 and 662 with nIter 1 on this input (192 individuals, seed 41)."""
    want, _ = _against_oracle(engine, _with_rare_sites(300, 192, 41))
    assert np.count_nonzero(want["n_iter"] == 0) > 0 and np.count_nonzero(want["n_iter"] == 1) > 0


def test_pairs_that_leave_at_iteration_0_at_eight_slots(engine):
    """500 individuals, seed 41: 774 pairs with nIter 0."""
    want, _ = _against_oracle(engine, _with_rare_sites(300, 500, 41))
    assert np.count_nonzero(want["n_iter"] == 0) > 0


@pytest.mark.parametrize("skip_marks", [False, True])
def test_sites_that_take_no_part(skip_marks):
    """A SNP-called matrix, handed over normalised (ngsld_set_geno_lkl), in which three sites are monomorphic (frequency 0),
    two hold triples that sum to 0.9 and one holds an individual whose likelihoods are all 0 (u . a == 0: every pair of the
    site is NaN in the reference).  All pairs meet the oracle; the pairs of those six sites are the same bits with the step on
    and off, and nIter is the same on every pair.  skip_marks: with site_skip_kernel's marks on (NGSLD_REPLAY_SKIP unset) the
    monomorphic sites are marked degenerate and the launch is the kernel's SKIP variant, which takes the step like the plain
    one on every pair it computes.  In both cases the step must have been taken: it moves last bits on some untouched pair."""
    raw = synth.make_gl_numpy(300, 192, 1301, depth=8.0)
    mono, odd, zero = [7, 150, 151], [20, 290], 40
    raw[mono] = (1.0, 0.0, 0.0)
    o = orc.Oracle(raw, n_threads=16)
    assert np.all(o.maf[mono] == 0.0)
    for s in odd:
        o.gl[s, 3::17] *= 0.9
        o.expg[s] = o.gl[s, :, 1] + 2 * o.gl[s, :, 2]
    o.gl[zero, 5] = 0.0
    o.expg[zero, 5] = 0.0
    want = o.run()
    touched = np.isin(want["s1"], mono + odd + [zero]) | np.isin(want["s2"], mono + odd + [zero])
    assert np.all(np.isnan(want["hap"][(want["s1"] == zero) | (want["s2"] == zero)]))
    old = os.environ.get("NGSLD_REPLAY_SKIP")
    if not skip_marks:
        os.environ["NGSLD_REPLAY_SKIP"] = "0"
    try:
        eng = capi.Engine(0)
    finally:
        if not skip_marks:
            if old is None:
                del os.environ["NGSLD_REPLAY_SKIP"]
            else:
                os.environ["NGSLD_REPLAY_SKIP"] = old
    try:
        on = _run(eng, lambda e: e.set_geno_lkl(o.gl, o.maf), None, True)
        off = _run(eng, lambda e: e.set_geno_lkl(o.gl, o.maf), None, False)
    finally:
        eng.close()
    for got in (on, off):
        assert np.array_equal(got[0], want["s1"]) and np.array_equal(got[1], want["s2"])
        check_records(got[2], got[3], want)
    assert np.array_equal(on[3]["n_iter"], off[3]["n_iter"])
    for name, where in VALUES:
        a, b = (on[3] if where == "ext" else on[2])[name], (off[3] if where == "ext" else off[2])[name]
        assert np.all(same_bits(a[touched], b[touched])), name
    assert _differ(on, off)[~touched].any(), "the first step from dosages was not taken on any pair"


def test_knob_parity_at_size(engine):
    """2,000 sites x 500 individuals, 100 kb window (the headline's shape): step on against step off, nIter equal on every
    record, values inside the suite's bar."""
    n_sites = 2000
    raw = synth.make_gl_numpy(n_sites, 500, 1401, depth=10.0)
    chrs, pos = synth.make_positions(n_sites, 1401, max_gap=200)
    pd = shard.pos_dist_from_positions(chrs, pos)
    on = _run(engine, lambda e: e.set_geno_raw(raw), pd, True, max_kb_dist=100)
    off = _run(engine, lambda e: e.set_geno_raw(raw), pd, False, max_kb_dist=100)
    assert len(on[0]) > 1_000_000
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[3]["n_iter"], off[3]["n_iter"]) and np.array_equal(on[3]["n_ind_data"], off[3]["n_ind_data"])
    for name, where in VALUES:
        a, b = (on[3] if where == "ext" else on[2])[name], (off[3] if where == "ext" else off[2])[name]
        ok = close(a, b, TOL)
        with np.errstate(invalid="ignore"):
            print(f"{name}: largest |on - off| = {np.nanmax(np.abs(a - b)):.3e}")
        assert np.all(ok), f"{name}: {np.count_nonzero(~ok)} values differ by more than {TOL}"
    assert _differ(on, off).any(), "the first step from dosages was not taken on any pair"
