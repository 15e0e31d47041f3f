"""LD decay on the host, no GPU: tests/decay_ref.py (the restatement of fit_LDdecay.R's binning) on hand-written tables, and
ngsld_host_decay_fit (capi.decay_fit) -- known curves recovered, no worse than a multi-start bounded minimiser of the script's
own sum of squares, inside the bounds, deterministic, and every invalid combination refused."""
import math
from fractions import Fraction

import numpy as np
import pytest

import decay_ref
from ngsld_amd import capi

HEAD = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\n"
HEAD_EXT = "site1\tsite2\tdist\tr2_ExpG\tD\tDp\tr2\tsample_size\tmaf1\tmaf2\n"


def _row(dist, r2_expg="0.100000", d="0.010000", dp="0.500000", r2="0.200000", maf=None):
    cells = ["a:1", "a:2", dist, r2_expg, d, dp, r2]
    if maf is not None:
        cells += ["10", maf[0], maf[1]]
    return "\t".join(cells) + "\n"


def test_bins_are_right_closed_and_labelled_by_the_lower_break():
    text = HEAD + _row("250", r2="0.300000") + _row("251", r2="0.100000") + _row("500", r2="0.200000") + _row("1", r2="0.400000")
    got = decay_ref.decay_bins(text, bin_size=250)
    assert [(d, n) for d, n, _ in got] == [(0.0, 2), (250.0, 2)]
    assert got[0][2]["r2"] == Fraction("0.35") and got[1][2]["r2"] == Fraction("0.15")


def test_dist_zero_falls_in_no_bin_and_empty_bins_do_not_appear():
    text = HEAD + _row("0") + _row("1000") + _row("1001")
    got = decay_ref.decay_bins(text, bin_size=250)
    assert [(d, n) for d, n, _ in got] == [(750.0, 1), (1000.0, 1)]


def test_the_distance_limit_is_strict():
    text = HEAD + _row("100") + _row("2000") + _row("1999") + _row("inf")
    got = decay_ref.decay_bins(text, bin_size=250, max_kb_dist=2)
    assert sum(n for _, n, _ in got) == 2                       # 2000 == 2 kb * 1000 is out, inf never counts
    assert sum(n for _, n, _ in decay_ref.decay_bins(text, bin_size=250)) == 3


def test_nan_in_one_chosen_statistic_drops_the_row_from_both():
    text = HEAD + _row("100", r2="-nan", dp="0.500000") + _row("120", r2="0.300000", dp="0.700000")
    got = decay_ref.decay_bins(text, ld=("r2", "Dp"), bin_size=250)
    assert got == [(0.0, 1, {"Dp": Fraction("0.7"), "r2": Fraction("0.3")})]
    got = decay_ref.decay_bins(text, ld=("Dp",), bin_size=250)     # not chosen: the row stays
    assert got == [(0.0, 2, {"Dp": Fraction("0.6")})]


def test_inf_text_is_dropped_like_nan():
    text = HEAD + _row("100", dp="inf") + _row("110", dp="-inf") + _row("120", dp="0.250000")
    got = decay_ref.decay_bins(text, ld=("Dp",), bin_size=250)
    assert got == [(0.0, 1, {"Dp": Fraction("0.25")})]


def test_min_maf_uses_the_printed_maf_columns():
    text = HEAD_EXT + _row("100", maf=("0.050000", "0.300000")) + _row("110", maf=("0.100000", "0.100000")) + \
        _row("120", maf=("-nan", "0.400000"))
    assert sum(n for _, n, _ in decay_ref.decay_bins(text, min_maf=0.1)) == 1
    assert sum(n for _, n, _ in decay_ref.decay_bins(text, min_maf=0.0)) == 2   # (a NaN maf never passes)


def test_fractional_bin_size_labels():
    text = HEAD + _row("62") + _row("63") + _row("125") + _row("126")
    got = decay_ref.decay_bins(text, bin_size=62.5)
    assert [(d, n) for d, n, _ in got] == [(0.0, 1), (62.5, 2), (125.0, 1)]


# ---- the fit ----

D = np.arange(0, 300) * 250.0


def _curve(field, rate, h, l, d=D, n_ind=0, rr=1.0):
    return decay_ref.model(field, rate, h, l, d, n_ind, rr)


@pytest.mark.parametrize("field,rate,h,l", [("r2", 3e-4, 0.8, 0.1), ("r2_ExpG", 2e-5, 0.6, 0.05), ("r2", 1e-3, 0.5, 0.0),
                                            ("r2", 5e-4, 1.0, 0.2)])
def test_recovers_the_three_parameter_r2_curve(field, rate, h, l):
    fit = capi.decay_fit(D, _curve(field, rate, h, l), field)
    assert fit["rate"] == pytest.approx(rate, rel=1e-6)
    assert fit["ld_max"] == pytest.approx(h, rel=1e-6, abs=1e-9) and fit["ld_min"] == pytest.approx(l, rel=1e-6, abs=1e-9)
    assert fit["sse"] < 1e-20 and fit["n_bins"] == len(D)


@pytest.mark.parametrize("rate,n_ind", [(3e-4, 50), (2e-3, 10), (5e-5, 500)])
def test_recovers_the_n_ind_curve(rate, n_ind):
    fit = capi.decay_fit(D, _curve("r2", rate, 0, 0, n_ind=n_ind), "r2", n_ind=n_ind)
    assert fit["rate"] == pytest.approx(rate, rel=1e-6)
    assert fit["ld_max"] == 0 and fit["ld_min"] == 0


@pytest.mark.parametrize("t,h,l,rr", [(30.0, 0.9, 0.2, 1.0), (4.0, 0.7, 0.0, 1.0), (120.0, 1.0, 0.3, 0.5)])
def test_recovers_the_dp_curve(t, h, l, rr):
    d = np.arange(0, 400) * 1000.0
    fit = capi.decay_fit(d, _curve("Dp", t, h, l, d=d, rr=rr), "Dp", recomb_rate=rr)
    assert fit["rate"] == pytest.approx(t, rel=1e-6)
    assert fit["ld_max"] == pytest.approx(h, rel=1e-6, abs=1e-9) and fit["ld_min"] == pytest.approx(l, rel=1e-6, abs=1e-9)


def _dp_tmax(d, rr):
    x = 1 - d * rr / 1e6
    g = -np.log(x[(x < 1) & (x > 0)]).min()
    return 50 / g


def _scipy_best(field, d, y, n_ind=0, rr=1.0, starts=24, seed=0):
    from scipy.optimize import minimize
    rng = np.random.default_rng(seed)
    if n_ind:
        f = lambda p: decay_ref.sse(field, (p[0], 0, 0), d, y, n_ind, rr)  # noqa: E731
        best = math.inf
        for _ in range(starts):
            r = minimize(f, [rng.uniform(0, 0.01)], method="L-BFGS-B", bounds=[(0, 1)])
            best = min(best, f(np.clip(r.x, 0, 1)))
        return best
    hi = _dp_tmax(d, rr) if field == "Dp" else 1.0
    f = lambda p: decay_ref.sse(field, p, d, y, n_ind, rr)  # noqa: E731
    best = math.inf
    for _ in range(starts):
        x0 = [rng.uniform(0, min(hi, 50.0) if field == "Dp" else 0.01), *sorted(rng.uniform(0, 1, 2))[::-1]]
        r = minimize(f, x0, method="SLSQP", bounds=[(0, hi), (0, 1), (0, 1)],
                     constraints=[{"type": "ineq", "fun": lambda p: p[1] - p[2]}], options={"maxiter": 500, "ftol": 1e-15})
        p = np.clip(r.x, [0, 0, 0], [hi, 1, 1])
        if p[1] < p[2]:
            p[1] = p[2] = (p[1] + p[2]) / 2
        best = min(best, f(p))
    return best


NOISY = [("r2", 3e-4, 0.8, 0.1, 0, 0.02), ("r2_ExpG", 1e-4, 0.5, 0.05, 0, 0.01), ("r2", 2e-3, 0.3, 0.25, 0, 0.05),
         ("r2", 3e-4, 0, 0, 40, 0.01), ("Dp", 20.0, 0.9, 0.1, 0, 0.03), ("Dp", 2.0, 0.6, 0.4, 0, 0.05)]


@pytest.mark.parametrize("k", range(len(NOISY)))
def test_noisy_fit_is_no_worse_than_a_multi_start_minimiser(k):
    field, rate, h, l, n_ind, sd = NOISY[k]
    d = np.arange(0, 200) * (1000.0 if field == "Dp" else 250.0)
    y = _curve(field, rate, h, l, d=d, n_ind=n_ind) + np.random.default_rng(k).normal(0, sd, len(d))
    fit = capi.decay_fit(d, y, field, n_ind=n_ind)
    want = _scipy_best(field, d, y, n_ind=n_ind, seed=k)
    assert fit["sse"] <= want + 1e-12 * max(1.0, fit["sse"]), (fit, want)
    assert fit["sse"] == pytest.approx(decay_ref.sse(field, (fit["rate"], fit["ld_max"], fit["ld_min"]), d, y, n_ind), rel=1e-12)
    hi = _dp_tmax(d, 1.0) if field == "Dp" else 1.0
    assert 0 <= fit["rate"] <= hi
    assert 0 <= fit["ld_min"] <= fit["ld_max"] <= 1


@pytest.mark.parametrize("seed", range(12))
def test_bounds_hold_on_any_data(seed):
    rng = np.random.default_rng(seed)
    d = np.sort(rng.choice(np.arange(0, 2000), 40, replace=False)) * 250.0
    y = rng.uniform(-0.5, 1.5, len(d)) if seed % 2 else rng.uniform(0, 1, len(d))[::-1].copy()
    for field in ("r2", "r2_ExpG", "Dp"):
        fit = capi.decay_fit(d, y, field)
        assert 0 <= fit["ld_min"] <= fit["ld_max"] <= 1 and fit["rate"] >= 0
        if field != "Dp":
            assert fit["rate"] <= 1
    fit = capi.decay_fit(d, y, "r2", n_ind=30)
    assert 0 <= fit["rate"] <= 1 and fit["ld_max"] == fit["ld_min"] == 0


def test_repeated_calls_are_bit_identical():
    y = _curve("r2", 3e-4, 0.8, 0.1) + np.random.default_rng(5).normal(0, 0.02, len(D))
    a = [capi.decay_fit(D, y, f) for f in ("r2", "Dp")]
    for _ in range(3):
        assert [capi.decay_fit(D, y, f) for f in ("r2", "Dp")] == a


@pytest.mark.parametrize("args,kw", [
    ((D, _curve("r2", 1e-4, 0.5, 0.1), "D"), {}),                       # D has no model
    ((D, _curve("r2", 1e-4, 0.5, 0.1), "Dp"), dict(n_ind=20)),          # n_ind with Dp
    ((np.array([]), np.array([]), "r2"), {}),                           # no bins
    ((np.array([0.0, 2e6]), np.array([0.5, 0.1]), "Dp"), {}),           # d * rr / 1e6 > 1: the curve is NaN
    ((np.array([0.0, 6e5]), np.array([0.5, 0.1]), "Dp"), dict(recomb_rate=2.0)),
    ((np.array([0.0, 250.0]), np.array([0.5, np.nan]), "r2"), {}),      # a non-finite input
    ((np.array([0.0, np.inf]), np.array([0.5, 0.1]), "r2"), {}),
    ((np.array([0.0, -250.0]), np.array([0.5, 0.1]), "r2"), {}),
    ((D, _curve("r2", 1e-4, 0.5, 0.1), "r2"), dict(n_ind=-1)),
    ((D, _curve("r2", 1e-4, 0.5, 0.1), "r2"), dict(recomb_rate=0.0)),
])
def test_invalid_combinations_are_refused(args, kw):
    with pytest.raises(capi.NgsldError) as e:
        capi.decay_fit(*args, **kw)
    assert e.value.code == capi.ERR_INVALID


def test_dp_at_exactly_one_is_accepted():
    d = np.array([0.0, 250.0, 1e6])
    fit = capi.decay_fit(d, np.array([0.9, 0.8, 0.1]), "Dp")
    assert 0 <= fit["ld_min"] <= fit["ld_max"] <= 1
