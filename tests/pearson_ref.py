"""Inputs on which r2_ExpG has no rounding to hide behind, and its prediction in plain numpy (no GPU, no library).

Every pair kernel forms a Pearson cross moment sxy = sum (e1 - mean1)(e2 - mean2) -- centred per element, or sum e1 e2 less
n mean1 mean2, on the vector pipe, read off the P products, or on the f64 matrix pipe (ld_pair_moments.hip) -- and hands it to
write_pair (ld_em.h): r = (sxy * |rsx1|) * |rsx2|, r2_ExpG = r * r.  exact_sites / exact_called_sites build inputs on which
that moment is EXACT in every one of those forms, so all of them must give the bits predict_r2 gives; graded_sites builds
real-valued inputs of graded variance, on which a kernel's distance from the reference is held to write_pair's own text margin
(text_margin).  tests/test_pearson_ref.py holds the builders to what they promise here."""
from __future__ import annotations

import numpy as np

CENTRES = (0.5, 0.75, 1.25, 1.5)
A1 = 0.125           # the heterozygote's likelihood of every individual of exact_sites
GRID = 2.0 ** -9     # the grid of its expected genotypes
PEARSON_COND = 2.0 ** 13   # kPearsonCond (ld_common.h): beyond it the pair is replayed, whatever the kernel computed
ULP = 2.0 ** -52


def exact_sites(n_sites: int, n_ind: int, seed: int, missing: int = 0):
    """(gl[n_sites, n_ind, 3], E[n_sites, n_ind], c[n_sites]): likelihood triples, their expected genotypes e = a1 + 2 a2 and the
    sites' centres, built so that the Pearson moment of any two sites is exact in any summation order.

    Construction.  a1 = 2^-3 for everybody; e = c + k 2^-9 with an integer k = sign * (|q| K // 128), |q| <= 127 the
    individual's step on a grid of 128 and K = 2^(7 - s % 8) the site's scale: eight scales per block of eight sites, from 127
    grid steps down to none (the scale-1 sites are constant: rsx = inf, r2_ExpG NaN -- kept, the constant site is an edge of its
    own).  c cycles through 0.5, 0.75, 1.25, 1.5 by (s // 8) % 4: half the sites have a frequency above 1/2 and are relabelled
    by the kernels.  a2 = (e - a1) / 2, a0 = 1 - a1 - a2: all in [2^-4, 0.8125], and (a0 + a1) + a2 == 1.0 exactly, so the
    quotient path of the prep kernel (a_g = raw_g * (1 / sum)) hands the values on unchanged.  Individuals come in (q, -q) pairs
    at shuffled positions (an odd n_ind leaves one individual at q = 0), so sum e = n c exactly and mean == c in any order.
    Site s + 1 keeps site s's |q| and signs but for a random 15 % of the pairs, drawn anew: neighbouring sites are in LD, and
    r2 runs from 0 to about 0.9.

    missing > 0 (for --ignore_miss_data): that many individuals carry the raw triple (0.25, 0.25, 0.25) at every site -- gl holds
    it as it is, raw.  The quotient path gives RN(1/3) three times, and fma(2, a, a) = RN(3 RN(1/3)) is exactly 1.0 under either
    label: 3 RN(1/3) = 1 - 2^-54 is a tie, and it rounds to even.  Each of them is balanced by a partner at e = 2c - 1, and only
    the centres 0.75 and 1.25 are used (c by (s // 8) % 2), where that partner is a valid triple.

    Why nothing rounds.  Every likelihood is a multiple of 2^-10 (e is one of 2^-9, a1 = 2^-3, a2 = (e - a1) / 2), at most 1.
    Every product a_g b_h, e1 e2 or (e1 - c1)(e2 - c2) is therefore a multiple of 2^-20 below 4, and so are 2 (P5 + P7) and 4 P8
    of the moment read off the P products (moment_of_P: (a1 + 2 a2)(b1 + 2 b2) = P4 + 2 (P5 + P7) + 4 P8).  Every partial sum of
    such terms, in whatever order and grouping, is a multiple of 2^-20 below 2^15 in magnitude for n_ind <= 2^13: 35 bits, inside
    the 53 of a double -- so no addition rounds, with or without fused multiply-add (an FMA rounds once, and here not at all),
    in sequential, tree, chunked or matrix-pipe order (v_mfma_f64_16x16x4_f64 is a chain of FMAs).  n c1 c2 is an integer below
    2^13 times a multiple of 2^-4: exact, and so is its subtraction from sum e1 e2.  The relabelled 2 - e and 2 - mean are exact
    too, and a1 + 2 a0 IS 2 - e because the triple sums to 1.  sum e = n c is exact and n c / n == c, a correctly rounded
    quotient of an exact one; sq = sum (e - c)^2 is exact like the moment.  rsx = 1 / sqrt(sq) is two correctly rounded
    operations on the device and in numpy alike: the same bits.  What is left of r2_ExpG are three correctly rounded products,
    (sxy * rsx1) * rsx2 and r * r: the same bits wherever sxy is exact."""
    assert 0 < n_ind <= 2 ** 13 and 0 <= 2 * missing <= n_ind
    rng = np.random.default_rng(seed)
    free = n_ind - 2 * missing
    n_pairs = free // 2
    order = rng.permutation(n_ind)
    miss_at, partner_at = order[:missing], order[missing:2 * missing]
    plus_at, minus_at = order[2 * missing:2 * missing + n_pairs], order[2 * missing + n_pairs:2 * missing + 2 * n_pairs]
    centres = (0.75, 1.25) if missing else CENTRES
    q = rng.integers(0, 128, n_pairs)
    sign = rng.choice((-1, 1), n_pairs)
    E = np.empty((n_sites, n_ind))
    c = np.empty(n_sites)
    for s in range(n_sites):
        if s:
            anew = rng.random(n_pairs) < 0.15
            q = np.where(anew, rng.integers(0, 128, n_pairs), q)
            sign = np.where(anew, rng.choice((-1, 1), n_pairs), sign)
        scale = 2 ** (7 - s % 8)
        k = sign * (q * scale // 128)
        c[s] = centres[(s // 8) % len(centres)]
        E[s] = c[s]  # (the odd individual, if any, stays here)
        E[s, plus_at] = c[s] + k * GRID
        E[s, minus_at] = c[s] - k * GRID
        E[s, partner_at] = 2 * c[s] - 1
        E[s, miss_at] = 1.0
    gl = np.empty((n_sites, n_ind, 3))
    gl[:, :, 1] = A1
    gl[:, :, 2] = (E - A1) / 2
    gl[:, :, 0] = 1 - gl[:, :, 1] - gl[:, :, 2]
    gl[:, miss_at] = 0.25
    return gl, E, c


# called genotypes of four individuals whose sum is 4 c: the slots exact_called_sites fills
_SLOTS = {
    0.5: ((0, 0, 0, 2), (0, 1, 0, 1)),            # (0, 0, 0, 2), or (0, 1) twice
    1.0: ((0, 2, 0, 2), (0, 2, 1, 1), (1, 1, 1, 1)),  # (0, 2) and (1) put together
    1.5: ((2, 2, 2, 0), (2, 1, 2, 1)),            # the mirror images of 0.5
}
_TAIL = {0.5: (0, 1), 1.0: (0, 2), 1.5: (2, 1)}   # two individuals left over by an n_ind that is 2 mod 4


def exact_called_sites(n_sites: int, n_ind: int, seed: int):
    """(raw[n_sites, n_ind, 3], E, c) for the called-genotype kernel (pair_ld_hard_kernel): likelihood 1 for the called
    genotype and 0 elsewhere, fed as tests/test_gpu_hardcalls.py feeds its inputs.  Genotypes come in groups whose mean is the
    site's centre -- (0, 1) and (0, 0, 0, 2) for 0.5; (0, 2) and (1) for 1.0; the mirror images for 1.5 -- here as slots of
    four individuals at shuffled positions, each slot one of the combinations of those groups, in a random order.  The centre
    changes every eight sites (0.5, 1.0, 1.5 by (s // 8) % 3); within such a block site s + 1 keeps site s's slots but for a
    random 15 %.  e is 0, 1 or 2 and c a multiple of 1/2: every term of every form of the moment is a multiple of 1/4, exact like
    exact_sites' and with less to spare.  n_ind must be even (a mean of 0.5 over an odd number of called genotypes is impossible)."""
    assert n_ind % 2 == 0 and 0 < n_ind <= 2 ** 13
    rng = np.random.default_rng(seed)
    order = rng.permutation(n_ind)
    n_slots = n_ind // 4
    G = np.empty((n_sites, n_ind), dtype=np.int64)
    c = np.empty(n_sites)
    slots = None
    for s in range(n_sites):
        c[s] = (0.5, 1.0, 1.5)[(s // 8) % 3]
        kinds = _SLOTS[c[s]]
        fresh = np.array([rng.permutation(kinds[rng.integers(len(kinds))]) for _ in range(n_slots)]).reshape(n_slots, 4)
        if s % 8 == 0:
            slots = fresh
        else:
            slots = np.where((rng.random(n_slots) < 0.15)[:, None], fresh, slots)
        G[s, order[:4 * n_slots]] = slots.reshape(-1)
        if n_ind % 4:
            G[s, order[4 * n_slots:]] = _TAIL[c[s]]
    return np.eye(3)[G], G.astype(np.float64), c


def predict_r2(E: np.ndarray, maf: np.ndarray, s1: np.ndarray, s2: np.ndarray) -> np.ndarray:
    """r2_ExpG of the pairs (s1, s2) from the expected genotypes E[n_sites, n_ind], in the device's steps: a site's mean
    (ld_prep.hip: sum e / n, or the common value of a constant site) and sq = sum (e - mean)^2, rsx = 1 / sqrt(sq); the
    relabelling of a site whose frequency is above 1/2 (2 - e, 2 - mean: Relabel); sxy = sum e1 e2 - n mean1 mean2;
    r = (sxy * rsx1) * rsx2 and r * r (write_pair).  NaN where either site is constant.  On exact_sites' inputs every step in front
    of rsx is exact, so these are the bits every kernel family must give; on others it is one more f64 evaluation."""
    E = np.asarray(E, dtype=np.float64)
    n = E.shape[1]
    s1, s2 = np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)
    flip = np.asarray(maf) > 0.5
    El = np.where(flip[:, None], 2.0 - E, E)
    constant = El.min(axis=1) == El.max(axis=1)
    mean = np.where(constant, El[:, 0], El.sum(axis=1) / n)
    d = El - mean[:, None]
    sq = (d * d).sum(axis=1)
    with np.errstate(divide="ignore"):
        rsx = 1.0 / np.sqrt(sq)
    out = np.empty(len(s1))
    for lo in range(0, len(s1), 1 << 16):
        a, b = s1[lo:lo + (1 << 16)], s2[lo:lo + (1 << 16)]
        sxy = np.einsum("ki,ki->k", El[a], El[b]) - (n * mean[a]) * mean[b]
        with np.errstate(invalid="ignore"):
            r = (sxy * rsx[a]) * rsx[b]
            out[lo:lo + (1 << 16)] = r * r
    out[constant[s1] | constant[s2]] = np.nan
    return out


def graded_sites(n_sites: int, n_ind: int, seed: int) -> np.ndarray:
    """raw[n_sites, n_ind, 3]: real-valued likelihoods whose expected genotypes have a graded spread, for the text margin.
    e = centre + 0.4 * 2^-(s % 8) * z with z uniform in [-1, 1], the centre 0.6 or 1.4 by (s // 8) % 2; p1 = 0.2,
    p2 = (e - p1) / 2, p0 = 1 - p1 - p2; each triple is then scaled by a factor drawn from [0.5, 2], so the input is raw and
    un-normalised.  std(e) = 0.23 * 2^-(s % 8): the pairs' 1 / (std1 std2) runs from 2^4.2 to 2^18.2 in steps of an octave, two
    thirds of them at or below kPearsonCond = 2^13 (the sums of two scale indices up to 8: 43 of the 64 combinations)."""
    rng = np.random.default_rng(seed)
    s = np.arange(n_sites)
    z = rng.uniform(-1.0, 1.0, (n_sites, n_ind))
    e = np.where((s // 8) % 2 == 0, 0.6, 1.4)[:, None] + (0.4 * 2.0 ** -(s % 8))[:, None] * z
    raw = np.empty((n_sites, n_ind, 3))
    raw[:, :, 1] = 0.2
    raw[:, :, 2] = (e - 0.2) / 2
    raw[:, :, 0] = 1 - raw[:, :, 1] - raw[:, :, 2]
    return raw * rng.uniform(0.5, 2.0, (n_sites, n_ind))[:, :, None]


def pair_cond(expg: np.ndarray, s1: np.ndarray, s2: np.ndarray) -> np.ndarray:
    """1 / (std1 std2) of the pairs from expected genotypes (the oracle's expg): write_pair's cond = n |rsx1| |rsx2|."""
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.std(np.asarray(expg, dtype=np.float64), axis=1)
    return inv[np.asarray(s1, dtype=np.int64)] * inv[np.asarray(s2, dtype=np.int64)]


def text_margin(cond: np.ndarray, from_pass: bool) -> np.ndarray:
    """write_pair's text margin of r2_ExpG, d_abs * fma(half_kn, cond, 0.5): 32 ulp * (k cond + 0.5) with k = 6 where
    pair_ld_moments_kernel supplied the moment and k = 2 elsewhere.  A pair closer than this to a sixth-decimal rounding point is
    flagged and replayed; a kernel further than this from the reference prints a wrong digit sooner or later."""
    return 32 * ULP * ((6.0 if from_pass else 2.0) * np.asarray(cond) + 0.5)


def adjacent_differ(r2: np.ndarray) -> float:
    """Share of the neighbouring records (k, k + 1), at least one of them finite, whose r2_ExpG differ in bits.  (Two NaN
    neighbours -- pairs of a constant site -- are NaN whatever moment reaches them: nothing of the map could show there.)"""
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    a, b = r2[:-1], r2[1:]
    counted = np.isfinite(a) | np.isfinite(b)
    differ = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return float(differ[counted].mean())
