"""CPU: tests/pearson_ref.py keeps its promises -- the moment of exact_sites' inputs is the same bits in every summation order
and form, predict_r2 agrees with the oracle, graded_sites fills the octaves of 1 / (std1 std2) the margin test walks through, and
the oracle's long-double recurrence is a reference far finer than the margin held against it."""
import numpy as np
import pytest

from oracle import orc
from pearson_ref import (PEARSON_COND, adjacent_differ, exact_called_sites, exact_sites, graded_sites, pair_cond, predict_r2,
                         text_margin)
from util import same_bits

N_SITES = 64
S1, S2 = (x.astype(np.int64) for x in np.triu_indices(N_SITES, 1))


def _seq(terms):
    """Sum over axis 1, one term after the other, every addition rounded on its own."""
    acc = np.zeros(terms.shape[0])
    for i in range(terms.shape[1]):
        acc = acc + terms[:, i]
    return acc


def _chunked(terms, chunk=16):
    """The order of pair_ld_moments_kernel: a chunk's terms added from zero, the chunks' sums added in order."""
    pad = (-terms.shape[1]) % chunk
    t = np.concatenate([terms, np.zeros((terms.shape[0], pad))], axis=1).reshape(terms.shape[0], -1, chunk)
    acc = np.zeros(terms.shape[0])
    for k in range(t.shape[1]):
        acc = acc + _seq(t[:, k])
    return acc


@pytest.mark.parametrize("n_ind,missing", [(61, 0), (500, 0), (576, 0), (5121, 0), (500, 50), (5121, 512)])
def test_moment_is_the_same_bits_in_every_order(n_ind, missing):
    gl, E, c = exact_sites(N_SITES, n_ind, 31 + n_ind, missing=missing)
    # the triples are what the docstring says: on the 2^-10 grid, in [2^-4, 0.8125], summing to 1.0 as the prep kernel adds them
    with_data = ~np.all(gl == 0.25, axis=(0, 2))
    triple = gl[:, with_data]
    assert triple.shape[1] == n_ind - missing
    assert np.all(triple * 1024 == np.round(triple * 1024)) and triple.min() >= 2.0 ** -4 and triple.max() <= 0.8125
    assert np.all((triple[:, :, 0] + triple[:, :, 1]) + triple[:, :, 2] == 1.0)
    assert np.all(triple[:, :, 1] + 2 * triple[:, :, 2] == E[:, with_data])
    if missing:  # the quotient path on (0.25, 0.25, 0.25): RN(1/3), and 3 RN(1/3) rounds to 1.0
        a = 0.25 * (1.0 / ((0.25 + 0.25) + 0.25))
        assert a == 1.0 / 3.0 and a + 2 * a == 1.0 and np.all(E[:, ~with_data] == 1.0)
        from fractions import Fraction
        assert 3 * Fraction(a) == 1 - Fraction(1, 2 ** 54)  # (the tie an FMA rounds to even: 1.0)
    # mean == c and sq, sequentially and pairwise
    assert np.all(_seq(E) == n_ind * c) and np.all(E.sum(axis=1) == n_ind * c) and np.all(n_ind * c / n_ind == c)
    d = E - c[:, None]
    assert np.all(_seq(d * d) == (d * d).sum(axis=1))
    # the moment four ways (and, without missing data, read off the P products as moment_of_P does)
    e1, e2, d1, d2 = E[S1], E[S2], d[S1], d[S2]
    ways = {
        "uncentred less n c1 c2": _seq(e1 * e2) - (n_ind * c[S1]) * c[S2],
        "centred per element": _seq(d1 * d2),
        "reversed": _seq((d1 * d2)[:, ::-1]),
        "chunks of 16": _chunked(e1 * e2) - (n_ind * c[S1]) * c[S2],
        "pairwise": (d1 * d2).sum(axis=1),
    }
    if not missing:
        a, b = gl[S1], gl[S2]
        p4, p5, p7, p8 = a[:, :, 1] * b[:, :, 1], a[:, :, 1] * b[:, :, 2], a[:, :, 2] * b[:, :, 1], a[:, :, 2] * b[:, :, 2]
        ways["off the P products"] = _seq(4.0 * p8 + (2.0 * (p5 + p7) + p4)) - (n_ind * c[S1]) * c[S2]
    first = ways["centred per element"]
    for name, got in ways.items():
        assert np.all(same_bits(got, first)), name
    # ... and under the other label
    assert np.all(same_bits(_seq((2 - e1) * (2 - e2)) - (n_ind * (2 - c[S1])) * (2 - c[S2]), first))
    # the prediction is that moment through write_pair's expression, whatever the labels
    sq = (d * d).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rsx = 1.0 / np.sqrt(sq)
        r = (first * rsx[S1]) * rsx[S2]
        want = r * r
    for maf in (np.zeros(N_SITES), np.ones(N_SITES), (c > 1).astype(float)):
        assert np.all(same_bits(predict_r2(E, maf, S1, S2), want))
    # the edges are there: constant sites (every eighth), NaN on all their pairs; r2 from 0 to 0.7 .. 0.9
    # (with missing individuals no site is constant: they and their partners stand apart from the centre)
    assert np.array_equal(np.flatnonzero(sq == 0), np.arange(0 if missing else 7, 0 if missing else N_SITES, 8))
    assert np.array_equal(np.isnan(want), (sq == 0)[S1] | (sq == 0)[S2])
    assert missing or (np.nanmin(want) < 1e-3 and 0.6 < np.nanmax(want) <= 1.0)  # (the missing and their partners correlate every pair)
    assert adjacent_differ(want) > 0.99


def test_called_sites_are_exact():
    raw, E, c = exact_called_sites(N_SITES, 250, 77)
    assert np.all(raw.sum(axis=2) == 1.0) and set(np.unique(raw)) == {0.0, 1.0} and set(np.unique(c)) == {0.5, 1.0, 1.5}
    assert np.all(raw[:, :, 1] + 2 * raw[:, :, 2] == E) and np.all(E.sum(axis=1) == 250 * c)
    d = E - c[:, None]
    assert np.all((d * d).sum(axis=1) > 0)
    want = predict_r2(E, np.zeros(N_SITES), S1, S2)
    assert np.all(np.isfinite(want)) and np.nanmax(want) > 0.3
    assert np.all(same_bits(want, predict_r2(E, np.ones(N_SITES), S1, S2)))


@pytest.mark.parametrize("n_ind,missing", [(61, 0), (500, 0), (576, 0), (5121, 0), (500, 50)])
def test_prediction_agrees_with_the_oracle(n_ind, missing):
    """The oracle normalises through log / exp, so its expected genotypes are not these bits: 1e-13 (largest seen: 8e-15)."""
    gl, E, _ = exact_sites(N_SITES, n_ind, 31 + n_ind, missing=missing)
    o = orc.Oracle(gl, ignore_miss_data=missing > 0, n_threads=4)
    want = o.run()
    assert np.array_equal(want["s1"].astype(np.int64), S1) and np.array_equal(want["s2"].astype(np.int64), S2)
    got = predict_r2(E, o.maf, S1, S2)
    finite = np.isfinite(got)
    assert finite.all() if missing else 0.7 < finite.mean() < 0.8
    diff = np.abs(got[finite] - want["r2pear"][finite])
    print(f"n_ind {n_ind} missing {missing}: largest |prediction - oracle| = {diff.max():.3e} on {finite.sum()} finite pairs")
    assert np.all(diff <= 1e-13)


def _two_pass_longdouble(expg, s1, s2):
    e = np.asarray(expg, dtype=np.longdouble)
    d = e - e.mean(axis=1)[:, None]
    sq = (d * d).sum(axis=1)
    sxy = np.array([(d[a] * d[b]).sum() for a, b in zip(s1, s2)], dtype=np.longdouble)
    r = sxy / np.sqrt(sq[s1] * sq[s2])
    return r * r


def test_graded_sites_keep_their_shape():
    raw = graded_sites(96, 500, 4)
    assert np.all(raw > 0) and not np.allclose(raw.sum(axis=2), 1.0)
    o = orc.Oracle(raw, n_threads=4)
    want = o.run()
    assert len(want) == 4560
    s1, s2 = want["s1"].astype(np.int64), want["s2"].astype(np.int64)
    cond = pair_cond(o.expg, s1, s2)
    held = np.isfinite(cond) & (cond <= PEARSON_COND)
    octave = np.floor(np.log2(cond))
    per_octave = {k: int(np.count_nonzero(held & (octave == k))) for k in range(4, 13)}
    print(f"held {held.mean():.3f} of {len(cond)} pairs; per octave of 1 / (std1 std2): {per_octave}")
    assert held.mean() >= 0.60 and min(per_octave.values()) >= 50 and sum(per_octave.values()) == held.sum()
    # the reference of the margin test: the oracle's long-double recurrence against a two-pass long-double evaluation
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        ld = _two_pass_longdouble(o.expg, s1, s2)
        ratio = (np.abs(want["r2pear"][held].astype(np.longdouble) - ld[held]) / text_margin(cond[held], False)).astype(np.float64)
        print(f"oracle against two-pass long double: largest |difference| / margin = {ratio.max():.3e}")
        assert ratio.max() <= 1e-4
