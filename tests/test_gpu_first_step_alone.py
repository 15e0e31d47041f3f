"""GPU: iteration 0 of the EM by itself -- the run kernel's first step from dosages (ld_kernel_run.h, site_dose_kernel in
ld_prep.hip, the FIRST branch of em_pair) and every other pair-kernel family's iteration 0 -- against an extended-precision
restatement of that one step (tests/first_step_ref.py; its construction is proved on the CPU in tests/test_first_step_ref.py).

tests/test_gpu_first_step.py sees the step through the end of the EM, a contraction that shrinks an error of the first step
with every later iteration.  On the input used here the pairs of sites from different groups leave the EM at iteration 0 in
the reference: their record is the first step and nothing else, at frequencies of 0.02 .. 0.7.

How the records are taken.  Every case loads the matrix twice per knob state.  With the exact-order replay on (the default),
all pairs go through check_records and nIter / sample_size are exact.  With the replay off (ngsld_set_replay) the records are
the kernel's own on every pair -- D of a cross-group pair is rounding noise around 0, which ngsld_run flags for the replay so
that "-0.000000" prints like the reference's; replayed, the pair would show the replay's arithmetic, not the kernel's -- and
the cross-group pairs are held to the long-double step.

The bar on a cross-group pair's four frequencies: 16 x max(the oracle's own worst deviation from the long-double step on the
same pairs, 2^-53), computed in the test from the reference alone.  The oracle divides once per individual, correctly
rounded; the kernel shares one Newton-refined reciprocal over a product tree of up to eight dens per lane: a few ulp per
quotient before the sum.  Measured on one MI355X (printed per case): the kernels' largest deviation is 2.08e-16 (257
individuals, step on; every case lies within 1.3e-16 .. 2.1e-16), where the oracle's own is 4e-16 .. 1.9e-15 and the bars are
6e-15 .. 3e-14.
"""
import contextlib
import os

import numpy as np
import pytest

import first_step_ref as fr
from ngsld_amd import capi, shard, synth
from test_gpu_first_step import _first_step
from util import check_records, same_bits

pytestmark = pytest.mark.gpu

N_SITES = 60
COLUMNS = (("hap", "ext"), ("D", "std"), ("Dp", "std"), ("r2", "std"), ("r2_ExpG", "std"))


@contextlib.contextmanager
def _replay(eng, on: bool):
    eng.set_replay(on)
    try:
        yield
    finally:
        eng.set_replay(True)


def _records(eng, o, step_on: bool, replay: bool, kernel: str, pd=None, **plan):
    """(s1, s2, std, ext) of all planned pairs of the normalised matrix o.gl at the frequencies o.maf."""
    with _replay(eng, replay):
        with _first_step(step_on):
            eng.set_geno_lkl(o.gl, o.maf)
        assert eng.pair_kernel() == kernel
        eng.set_pos_dist(pd)
        n = eng.plan(extend_out=True, **plan)
        got = eng.run()
    assert len(got[0]) == n
    return got


def _same(a, b, where=slice(None)) -> bool:
    """Two runs' records are the same bits in every column on the pairs `where`."""
    return all(np.all(same_bits((a[3] if w == "ext" else a[2])[name][where], (b[3] if w == "ext" else b[2])[name][where]))
               for name, w in COLUMNS)


class Held:
    """What one knob state of one case gave: `own`, the kernel's own records (replay off), and dev, their largest deviation
    from the long-double step on the cross-group pairs."""


def _hold(eng, inp, want, step_on: bool, kernel: str, label: str, pd=None, **plan) -> Held:
    o = inp.o
    x = inp.cross(want["s1"], want["s2"])
    assert x.sum() >= 50 and np.all(want["n_iter"][x] == 0)     # (the reference alone: tests/test_first_step_ref.py)
    step = inp.step(want["s1"][x], want["s2"][x])
    bar = 16 * max(fr.deviation(want["hap"][x], step), fr.ULP)
    h = Held()
    for replay in (True, False):
        s1, s2, std, ext = got = _records(eng, o, step_on, replay, kernel, pd, **plan)
        assert np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
        if replay:
            check_records(std, ext, want)                        # every pair, in-group pairs among them: nIter, sample_size exact
        else:
            h.own = got
            assert np.array_equal(ext["n_iter"][x], want["n_iter"][x]) and np.array_equal(ext["n_ind_data"], want["n_ind_data"])
            h.dev = fr.deviation(ext["hap"][x], step)
            print(f"{label}: kernel - long-double step = {h.dev:.3e} on {x.sum()} cross-group pairs (bar {bar:.3e}, "
                  f"oracle {bar / 16:.3e})")
            assert h.dev <= bar, f"{label}: {h.dev:.3e} above the bar {bar:.3e}"
    h.cross = x
    return h


@pytest.mark.parametrize("n_ind", [161, 192, 225, 256, 257, 320, 321, 384, 385, 448, 449, 512])
def test_every_slot_count_of_the_step(engine, n_ind):
    """Three to eight slots, the last one barely used (one individual, or 33 where 129..160 is another kernel's) and full.  Step
    on and off both meet the bar; they differ in some last bit on the cross-group pairs, so the step was taken there."""
    inp = fr.Input(N_SITES, n_ind)
    want = inp.o.run()
    assert capi.describe_dispatch(n_ind).split()[:2] == ["run", f"1x{(n_ind + 63) // 64}"]
    on = _hold(engine, inp, want, True, "run", f"n_ind {n_ind} step on")
    off = _hold(engine, inp, want, False, "run", f"n_ind {n_ind} step off")
    assert not np.all(same_bits(on.own[3]["hap"][on.cross], off.own[3]["hap"][on.cross])), "the first step from dosages was not taken"


@pytest.mark.parametrize("n_ind", [576, 640])
def test_no_step_at_nine_and_ten_slots(engine, n_ind):
    """The knob switches nothing: the same bits on every pair, and the per-individual step meets the same bar."""
    inp = fr.Input(N_SITES, n_ind)
    want = inp.o.run()
    assert capi.describe_dispatch(n_ind).split()[:2] == ["run", f"1x{n_ind // 64}"]
    on = _hold(engine, inp, want, True, "run", f"n_ind {n_ind} step on")
    off = _hold(engine, inp, want, False, "run", f"n_ind {n_ind} step off")
    assert _same(on.own, off.own)


@pytest.mark.parametrize("n_ind,family", [(100, "group"), (129, "group"), (700, "ab"), (1100, "multi")])
def test_iteration_0_of_the_other_families(engine, n_ind, family):
    """The lockstep kernel, the a/b form and two wavefronts per pair: the same input takes each out of its EM at iteration 0."""
    inp = fr.Input(N_SITES, n_ind)
    want = inp.o.run()
    assert capi.describe_dispatch(n_ind).split()[0] == family
    _hold(engine, inp, want, True, family, f"n_ind {n_ind} {family}")


def test_frequency_at_exactly_one_half(engine):
    """Relabel (m > 0.5) and site_dose_kernel must flip on the same side.  One site per group is mirror-symmetric, its fixed
    point 0.5 to the last bit; the two are handed 0.5 and its two neighbours.  Two more sites are handed 0.5 in all three runs
    with a dosage sum that is not n (first_step_ref.Input, tilted): at a site whose fixed point is 0.5 the sum is n under
    either labelling, and a flip on one side only cannot show."""
    inp = fr.Input(N_SITES, 257, mirror=True)
    assert np.all(inp.o.maf[inp.half + inp.tilted] == 0.5)
    for name, m in (("0.5", 0.5), ("0.5 + ulp", np.nextafter(0.5, 1.0)), ("0.5 - ulp", np.nextafter(0.5, 0.0))):
        inp.o.maf[inp.half] = m
        want = inp.o.run()
        on = _hold(engine, inp, want, True, "run", f"maf {name} step on")
        off = _hold(engine, inp, want, False, "run", f"maf {name} step off")
        assert np.count_nonzero(on.cross & (np.isin(want["s1"], inp.half) | np.isin(want["s2"], inp.half))) >= 58
        assert not np.all(same_bits(on.own[3]["hap"][on.cross], off.own[3]["hap"][on.cross]))


def test_candidate_sum_under_a_filtered_plan(engine):
    """Positions, --max_snp_dist, --rnd_sample and --min_maf together: the candidates of a row are no longer s1 + 1, s1 + 2, ...,
    and a dosage sum read for another site than the pair's shows at once."""
    n_ind = 500
    chrs, pos = synth.make_positions(N_SITES, 2500, max_gap=200)
    pd = shard.pos_dist_from_positions(chrs, pos)
    plan = dict(max_snp_dist=7, rnd_sample=0.5, seed=2500)
    inp = fr.Input(N_SITES, n_ind, pos_dist=pd, **plan)
    low = np.sort(inp.o.maf)
    min_maf = float(0.5 * (low[4] + low[5]))           # drops the five rarest sites
    inp.o.p.min_maf = min_maf
    want = inp.o.run()
    sites = set(want["s1"].tolist()) | set(want["s2"].tolist())
    assert 40 < len(want) < 300 and len(sites) <= N_SITES - 5
    on = _hold(engine, inp, want, True, "run", "filtered plan step on", pd, min_maf=min_maf, **plan)
    off = _hold(engine, inp, want, False, "run", "filtered plan step off", pd, min_maf=min_maf, **plan)
    assert not np.all(same_bits(on.own[3]["hap"][on.cross], off.own[3]["hap"][on.cross]))


def test_sanity_fallback():
    """Given frequencies that are NaN (a lane whose product of dens underflows) are dropped and the pair starts at iteration 0
    as it does without them.  Site marks off (NGSLD_REPLAY_SKIP=0), so that no mark pre-empts the pairs of site A.
    120 sites: A and its twin are the candidates of 118 and 119 rows.  Their pairs take 6 to 20 iterations, over which step on
    and step off arrive at the same bits on 97 pairs in 100 of any kind; measured, 5 of the twin's 119 pairs keep a difference
    (with 40 sites: none of 39, by that chance alone) and none of A's 118."""
    o, a, twin = fr.fallback_input(120)
    want = o.run()
    old = os.environ.get("NGSLD_REPLAY_SKIP")
    os.environ["NGSLD_REPLAY_SKIP"] = "0"
    try:
        eng = capi.Engine(0)
    finally:
        if old is None:
            del os.environ["NGSLD_REPLAY_SKIP"]
        else:
            os.environ["NGSLD_REPLAY_SKIP"] = old
    try:
        own = {}
        for step_on in (True, False):
            s1, s2, std, ext = _records(eng, o, step_on, True, "run")
            assert np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
            check_records(std, ext, want)
            own[step_on] = _records(eng, o, step_on, False, "run")
    finally:
        eng.close()
    cand_a, cand_twin = want["s2"] == a, want["s2"] == twin
    assert cand_a.sum() == 118 and cand_twin.sum() == 119
    for got in own.values():
        assert np.all(np.isfinite(got[3]["hap"])) and np.array_equal(got[3]["n_iter"][cand_a | cand_twin], want["n_iter"][cand_a | cand_twin])
    assert _same(own[True], own[False], cand_a)
    # such a site is dose_ok: its twin takes the step, so A's equality is the fallback's doing, not a flag's
    differ = ~np.all(same_bits(own[True][3]["hap"][cand_twin], own[False][3]["hap"][cand_twin]), axis=1)
    print(f"sanity fallback: {differ.sum()} of the twin's {cand_twin.sum()} pairs differ between step on and off, none of A's {cand_a.sum()}")
    assert differ.any()


def test_den_product_that_underflows_is_the_references_nan(engine):
    """Two sites of frequency 1e-85 share an individual who is certain hom-alt at both: the reference's s underflows to 0, four
    NaNs and nIter 0.  site_dose_kernel keeps such sites out of the step (a den below 2^-500), so the pair is the reference's,
    with the step on and off, bit for bit -- and so is every other pair of the two sites."""
    o = fr.underflow_input()
    want = o.run()
    a, b = fr.UNDERFLOW_SITES
    both = (want["s1"] == a) & (want["s2"] == b)
    of_sites = np.isin(want["s1"], (a, b)) | np.isin(want["s2"], (a, b))
    assert np.all(np.isnan(want["hap"][both])) and want["n_iter"][both][0] == 0 and of_sites.sum() == 75
    runs = {}
    for replay in (True, False):
        for step_on in (True, False):
            s1, s2, std, ext = runs[replay, step_on] = _records(engine, o, step_on, replay, "run")
            assert np.array_equal(s1, want["s1"]) and np.array_equal(s2, want["s2"])
            assert np.all(np.isnan(ext["hap"][both])) and ext["n_iter"][both][0] == 0, (replay, step_on, ext[both])
            if replay:
                check_records(std, ext, want)
        assert _same(runs[replay, True], runs[replay, False], of_sites)
