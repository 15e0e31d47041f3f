"""The first EM step alone: an input on which a pair's record IS iteration 0 of the EM at ordinary magnitudes, and a plain
extended-precision restatement of that step -- the yardstick of tests/test_gpu_first_step_alone.py, proved against the oracle
alone in tests/test_first_step_ref.py.

The input ("disjoint informative sets").  The individuals are dealt into two groups at random; site s is informative only for
the individuals of group s % 2, every other individual holds (1/3, 1/3, 1/3) there; every third site has its planes 0 and 2
swapped (a frequency above 1/2).  The frequencies handed over are each site's fixed point of m <- sum(d) / (2n), d the posterior
dosage under HWE weights at m (est_maf's value is up to 0.2 away from it on such sites).  For a pair of sites from different
groups every individual is uninformative at one of the two, its dosage there is 2m, sum d1 d2 = 4 n m1 m2, and the step from
linkage equilibrium moves nothing: the reference leaves its EM at iteration 0 and what it prints is one EM step from the
frequencies handed over.  Pairs inside a group are ordinary pairs.

The step, under the caller's labels (no relabelling), from the very doubles handed over:
  u = ((1-m)^2, 2m(1-m), m^2),  d = (u1 a1 + 2 u2 a2) / (u . a),  S = sum d,
  f3 = sum(d1 d2) / (4n),  f2 = S1 / (2n) - f3,  f1 = S2 / (2n) - f3,  f0 = 1 - f1 - f2 - f3
in np.longdouble where that carries 63 bits or more, in fractions.Fraction (dosages on a 2^-256 grid) where it does not.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from ngsld_amd import synth
from oracle import orc

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63     # x87 extended or better; otherwise the step is formed in exact rationals
ULP = 2.0 ** -53
EPSILON = 1e-5                      # the EM's convergence threshold (gen_func.cpp:1054)
TILT = 1e-3                         # e of a tilted site (Input): 1.5e-3 of dosage, 3e-6 of frequency at 257 individuals


def dosages(gl: np.ndarray, maf: np.ndarray) -> np.ndarray:
    """Posterior dosages [n_sites, n_ind] under HWE weights at maf, in long double."""
    a = np.asarray(gl, dtype=LD)
    m = np.asarray(maf, dtype=LD)[:, None]
    q = 1 - m
    u0, u1, u2 = q * q, 2 * m * q, m * m
    return (u1 * a[:, :, 1] + 2 * u2 * a[:, :, 2]) / (u0 * a[:, :, 0] + u1 * a[:, :, 1] + u2 * a[:, :, 2])


def fixed_point_maf(gl: np.ndarray, start: np.ndarray, tol: float = 1e-18, max_iter: int = 20000) -> np.ndarray:
    """Each site's fixed point of m <- sum(d(m)) / (2n), iterated in long double from `start` until no site moves by more than
    tol, rounded to double."""
    m = np.asarray(start, dtype=LD).copy()
    two_n = LD(2 * gl.shape[1])
    for _ in range(max_iter):
        new = dosages(gl, m).sum(axis=1) / two_n
        step = np.abs(new - m).max()
        m = new
        if step <= tol:
            break
    else:
        raise AssertionError(f"the frequency iteration still moves by {float(step):.3e} after {max_iter} steps")
    return m.astype(np.float64)


GRID = 1 << 256                     # (the exact path) dosages are rounded once to multiples of 2^-256: integer sums from there


def _step_exact(gl, maf, s1, s2):
    """The step in rationals, where long double is no wider than double: every dosage an exact quotient of exact sums of
    doubles, rounded to the 2^-256 grid (so that 500 of them add up as integers, not as fractions of 150,000 bits); the
    frequencies are rounded once, at the end."""
    n_ind = gl.shape[1]
    d = {}
    for s in sorted(set(s1.tolist()) | set(s2.tolist())):
        m = Fraction(float(maf[s]))
        u0, u1, u2 = (1 - m) ** 2, 2 * m * (1 - m), m * m
        d[s] = []
        for a in gl[s]:
            a0, a1, a2 = (Fraction(float(v)) for v in a)
            q = (u1 * a1 + 2 * u2 * a2) / (u0 * a0 + u1 * a1 + u2 * a2)
            d[s].append(q.numerator * GRID // q.denominator)
    S = {s: Fraction(sum(v), GRID) for s, v in d.items()}
    out = np.empty((len(s1), 4), dtype=LD)
    for k, (x, y) in enumerate(zip(s1.tolist(), s2.tolist())):
        f3 = Fraction(sum(p * q for p, q in zip(d[x], d[y])), GRID * GRID) / (4 * n_ind)
        f2 = S[x] / (2 * n_ind) - f3
        f1 = S[y] / (2 * n_ind) - f3
        for h, f in enumerate((1 - f1 - f2 - f3, f1, f2, f3)):
            hi = float(f)               # (correctly rounded; the remainder only adds something where long double is wider)
            out[k, h] = LD(hi) + LD(float(f - Fraction(hi)))
    return out


def one_step(gl: np.ndarray, maf: np.ndarray, s1, s2) -> np.ndarray:
    """hap[len(s1), 4] (long double) of ONE EM step from linkage equilibrium at maf, for the pairs (s1[k], s2[k])."""
    s1, s2 = np.asarray(s1, dtype=np.int64), np.asarray(s2, dtype=np.int64)
    if not WIDE:
        return _step_exact(gl, maf, s1, s2)
    n = LD(gl.shape[1])
    d = dosages(gl, maf)
    S = d.sum(axis=1)
    f3 = (d[s1] * d[s2]).sum(axis=1) / (4 * n)
    f2 = S[s1] / (2 * n) - f3
    f1 = S[s2] / (2 * n) - f3
    return np.stack([1 - f1 - f2 - f3, f1, f2, f3], axis=1)


def deviation(hap, step) -> float:
    """Largest |hap - step| over pairs and haplotypes (NaN anywhere: inf)."""
    d = np.abs(np.asarray(hap, dtype=LD) - step)
    return float("inf") if d.size and not np.all(np.isfinite(d)) else float(d.max()) if d.size else 0.0


class Input:
    """One built input: o (the oracle, its gl normalised and its maf overwritten with the fixed points), group[n_ind], and --
    mirror=True -- half[2], the sites (one per group) whose fixed point is 1/2 to the last bit, and tilted[2], two more whose
    fixed point is some 1e-5 above 1/2 and which are handed 0.5 all the same.  At a site whose fixed point is 1/2 the dosage sum
    is n under either labelling of its alleles, so a sum taken under the wrong labels cannot show there; at a tilted site it is
    off by 3e-3, while the step from 0.5 still moves the site's frequency by less than EPSILON (the pair ends at iteration 0)."""

    def __init__(self, n_sites: int, n_ind: int, data_seed: int | None = None, mirror: bool = False, pos_dist=None, **oracle_kw):
        seed = 2000 + n_ind if data_seed is None else data_seed
        rng = np.random.default_rng([seed, 0x646A])
        self.group = rng.permutation(n_ind) % 2
        raw = synth.make_gl_numpy(n_sites, n_ind, seed, depth=6.0)
        for s in range(n_sites):
            raw[s, self.group != s % 2] = 1.0 / 3.0
        raw[::3] = raw[::3, :, ::-1].copy()
        self.n_sites, self.n_ind = n_sites, n_ind
        o = self.o = orc.Oracle(raw, pos_dist, n_threads=oracle_kw.pop("n_threads", 8), **oracle_kw)
        self.half, self.tilted = [], []
        if mirror:
            for k, s in enumerate(range(n_sites // 2 + 1, n_sites // 2 + 5)):
                # mirror-symmetric in the normalised values: the second half of the site's informative individuals holds the
                # first half's triples with planes 0 and 2 swapped (an odd one out becomes uninformative)
                idx = np.flatnonzero(self.group == s % 2)
                h = len(idx) // 2
                flat = o.gl[s, np.flatnonzero(self.group != s % 2)[0]].copy()
                o.gl[s, idx[h:2 * h]] = o.gl[s, idx[:h], ::-1]
                if len(idx) > 2 * h:
                    o.gl[s, idx[-1]] = flat
                if k >= 2:  # tilted: one mirror couple becomes (c, c, c) and (c - e, c, c + e), dosages 1 and 1 + e / (2c) at 0.5
                    o.gl[s, idx[0]] = flat
                    o.gl[s, idx[h]] = flat + np.array([-TILT, 0.0, TILT])
                o.expg[s] = o.gl[s, :, 1] + 2 * o.gl[s, :, 2]
                (self.tilted if k >= 2 else self.half).append(s)
        self.est_maf = o.maf.copy()
        o.maf[:] = fixed_point_maf(o.gl, o.maf)
        self.fixed = o.maf.copy()
        o.maf[self.tilted] = 0.5

    def cross(self, s1, s2) -> np.ndarray:
        """Pairs of sites from different groups."""
        return (np.asarray(s1) % 2) != (np.asarray(s2) % 2)

    def step(self, s1, s2) -> np.ndarray:
        return one_step(self.o.gl, self.o.maf, s1, s2)


def _called(n_sites: int, n_ind: int, seed: int):
    return orc.Oracle(synth.make_gl_numpy(n_sites, n_ind, seed, depth=8.0), n_threads=8)


def _certain_hom_alt(o, site: int, individuals) -> None:
    o.gl[site, individuals] = (0.0, 0.0, 1.0)
    o.expg[site] = o.gl[site, :, 1] + 2 * o.gl[site, :, 2]


def fallback_input(n_sites: int = 40, n_ind: int = 300, seed: int = 3100):
    """An ordinary SNP-called matrix in which the last but one site, A, has frequency 1e-45 and four individuals who are
    certain hom-alt and share one lane of the run kernel (5, 69, 133, 197): each den = u . a is 1e-90 there, the lane's product
    of dens underflows and the frequencies given to the EM are NaN.  The last site is A's twin with the four on four lanes (6,
    71, 136, 201): a product of one such den and ordinary ones, the given frequencies are finite.  The reference is finite on
    every pair.  Returns (oracle, A, twin)."""
    o = _called(n_sites, n_ind, seed)
    a, twin = n_sites - 2, n_sites - 1
    o.gl[twin] = o.gl[a]
    _certain_hom_alt(o, a, [5, 69, 133, 197])
    _certain_hom_alt(o, twin, [6, 71, 136, 201])
    o.maf[[a, twin]] = 1e-45
    return o, a, twin


UNDERFLOW_SITES = (20, 37)


def underflow_input(n_ind: int = 300, seed: int = 3200):
    """An ordinary SNP-called matrix of 39 sites in which two sites (20, 37) have frequency 1e-85 and share one individual who
    is certain hom-alt at both: at each site his den is 1e-170, positive and finite, while the reference's s of the pair of
    the two -- their product -- underflows to 0: four NaNs and nIter 0 there, finite values on the other 74 pairs of the two."""
    o = _called(39, n_ind, seed)
    for s in UNDERFLOW_SITES:
        _certain_hom_alt(o, s, [7])
    o.maf[list(UNDERFLOW_SITES)] = 1e-85
    return o
