"""GPU: the device's own copies of "%f" -- the text formatter (ld_text.hip: put_fixed, format_row with the float chi2 of the
extended columns) and the printed-value quantiser that LD pruning and LD decay build into their kernels (ld_prune.h) -- against
printf and the host, on the values random data almost never produces: exact ties at the sixth decimal and their ulp
neighbours, signed zeros, subnormals, the formatter's limits, NaN and inf.  The rows go through the production passes
(ngsld_selftest_format), the quantiser through the same inline functions (ngsld_selftest_printed)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import printed_values as pv
from ngsld_amd import capi

pytestmark = pytest.mark.gpu


def _fast_values():
    """Every value the device formats in its fast path (the rest raise needs_host: test_needs_host_...)."""
    vals = (pv.tie_values() + pv.negative_zero_values() + pv.subnormal_values() + pv.nonfinite_values() + pv.limit_values() +
            pv.host_format_values()[::4])
    return [v for v in vals if not pv.needs_host(v)]


def _std(vals):
    vals = list(vals) + [0.0] * (-len(vals) % 4)
    rec = np.zeros(len(vals) // 4, dtype=capi.REC_STD)
    a = np.array(vals, dtype=np.float64).reshape(-1, 4)
    for k, f in enumerate(("r2_ExpG", "D", "Dp", "r2")):
        rec[f] = a[:, k]
    return rec, a


DISTS = [0.0, 1.0, 2.0, 0.5, 1.5, 2.5, 3.5, 1e6 + 0.5, 12345.0, 99999999.0, 2.0 ** 53, 2.0 ** 53 - 1, 4503599627370495.5,
         2.0 ** 62, float("inf")]


def _printf0(d: float) -> str:
    return "inf" if d == float("inf") else "%.0f" % d


def test_standard_rows_are_printf(engine):
    fast = _fast_values()
    rec, a = _std(fast)
    n = len(rec)
    dist = np.array([DISTS[i % len(DISTS)] for i in range(n)])
    rows, host = engine.selftest_format(rec, None, dist, 0.0, 0.0)
    assert not host, "needs_host raised though every value is inside the fast path"
    ties = 0
    for i in range(n):
        want = capi.format_pair(None, None, dist[i], rec[i], None, 0.0, 0.0)
        assert rows[i] == want, (i, rows[i], want)
        f = rows[i].rstrip("\n").split("\t")
        assert f[:2] == ["(null)", "(null)"] and f[2] == _printf0(dist[i]), (i, f[2], dist[i])
        assert f[3:] == [pv.printf_f(v) for v in a[i]], (i, f[3:], [repr(v) for v in a[i]])
        ties += int(pv.is_tie(a[i]).sum())
    assert ties >= 1000
    print(f"standard rows: {n} rows, {4 * n} values, {ties} exact ties, all printf")


def test_needs_host_exactly_beyond_the_fast_path(engine):
    """One row per value around the limit: needs_host is raised iff floor(|v| * 10^6) >= 2^63 (from ~9.22e12 on, so for
    every |v| >= 2^52), in any of the four fields; rows inside the limit equal the host's."""
    vals = pv.limit_values() + [2.0 ** 63, 1e22, -1e300, 1e12, -123456789.987654321]
    assert sum(map(pv.needs_host, vals)) >= 16 and sum(not pv.needs_host(v) for v in vals) >= 6
    for k, v in enumerate(vals):
        four = [0.25, 0.25, 0.25, 0.25]
        four[k % 4] = v
        rec, _ = _std(four)
        rows, host = engine.selftest_format(rec, None, [1.0], 0.0, 0.0)
        assert host == pv.needs_host(v), (repr(v), host)
        if not host:
            assert rows[0] == capi.format_pair(None, None, 1.0, rec[0], None, 0.0, 0.0)
    # the dist column ("%.0f") has a 63-bit quotient of its own: 2^62 fits, 2^63 does not
    rec, _ = _std([0.0] * 4)
    assert engine.selftest_format(rec, None, [2.0 ** 62], 0.0, 0.0)[1] is False
    assert engine.selftest_format(rec, None, [2.0 ** 63], 0.0, 0.0)[1] is True
    print(f"needs_host: {sum(map(pv.needs_host, vals))} values beyond the fast path, {sum(not pv.needs_host(v) for v in vals)} inside")


def _ext_cases():
    """(hap[4], n_ind_data, n_iter, maf1, maf2) of crafted extended rows."""
    tiny = [1e-20, 1e-25, 1e-30, 1e-38, 1e-39, 1e-40, 1e-42, 1e-44, 1e-45, 1e-46]
    one_up = pv.from_bits(pv.bits(1.0) + 1)
    cases = []
    for a in range(0, 65, 4):                                             # exact dyadics (ties among them: x / 128 sums)
        for b in range(0, 65 - a, 8):
            for c in range(0, 65 - a - b, 16):
                cases.append([a / 64, b / 64, c / 64, (64 - a - b - c) / 64])
    for x in (0.0, 1.0, 0.5, 3 / 128, 0.25):                              # freq_A / freq_B exactly 0 or 1: exp_hap 0 -> inf / NaN
        cases += [[0.0, 0.0, x, 1 - x], [x, 1 - x, 0.0, 0.0], [0.0, x, 0.0, 1 - x], [x, 0.0, 1 - x, 0.0]]
    for t in tiny:                                                        # subnormal / flushed float products
        cases += [[t, 0.0, 0.0, 1 - t], [t, t, t, 1.0], [0.0, t, 0.0, 1.0], [0.0, 0.0, t, 1.0], [1.0, 0.0, t, 0.0],
                  [t, 0.0, 0.0, 0.0], [t, 1e-20, 1e-20, 1.0]]
    cases += [[0.5, one_up - 0.5, 0.0, 0.0], [0.5, 0.5, 2.0 ** -53, 0.0], [one_up, 0.0, 0.0, 0.0], [0.25, 0.75, one_up - 0.25, 0.0],
              [pv.from_bits(pv.bits(0.5) + 1), 0.5, 0.5, 0.0], [1.0, 2.0 ** -52, 2.0 ** -52, 0.0]]   # hap sums an ulp above 1
    for t in pv.odd_128_ties(1.0)[::7]:
        for s in pv.ulp_steps(t, (-1, 0, 1)):
            cases.append([s, 0.5 - s if s < 0.5 else 0.0, 0.25, 0.25])
    cases += [[float("nan"), 0.5, 0.25, 0.25], [-0.0, 0.5, 0.5, 0.0], [-1e-7, 0.5, 0.5, 1e-7]]
    rng = np.random.default_rng(5)
    cases += [list(x) for x in rng.dirichlet([0.3, 0.3, 0.3, 0.3], size=300)]
    big = [0, 1, 2 ** 31, 2 ** 32 - 1, 4_294_967_294, 1000]
    mafs = [0.0, 1.0, 0.5, 3 / 128, -0.0, 5e-324, 0.9999995, 1 - 2.0 ** -53]
    return [(h, big[k % len(big)], big[(k // 2) % len(big)], mafs[k % len(mafs)], mafs[(k * 3 + 1) % len(mafs)])
            for k, h in enumerate(cases)]


def test_extended_rows_equal_the_host(engine):
    cases = _ext_cases()
    n = len(cases)
    ext = np.zeros(n, dtype=capi.REC_EXT)
    ext["hap"] = np.array([c[0] for c in cases])
    ext["n_ind_data"] = [c[1] for c in cases]
    ext["n_iter"] = [c[2] for c in cases]
    fast = _fast_values()
    rec, _ = _std((fast * (4 * n // len(fast) + 1))[:4 * n])
    maf1, maf2 = np.array([c[3] for c in cases]), np.array([c[4] for c in cases])
    dist = np.array([DISTS[i % len(DISTS)] for i in range(n)])
    rows, host = engine.selftest_format(rec, ext, dist, maf1, maf2)
    assert not host
    chi2_nonfinite = 0
    for i in range(n):
        want = capi.format_pair(None, None, dist[i], rec[i], ext[i], maf1[i], maf2[i])
        assert rows[i] == want, (i, cases[i], rows[i], want)
        chi2 = rows[i].split("\t")[16]
        chi2_nonfinite += chi2 in ("inf", "-nan")
    assert chi2_nonfinite >= 10
    print(f"extended rows: {n} rows equal to the host's, {chi2_nonfinite} with chi2 inf / -nan")


def _quantiser_values(every: int = 16):
    x = (pv.tie_values() + pv.negative_zero_values() + pv.subnormal_values() + pv.nonfinite_values() + pv.limit_values() +
         pv.host_format_values()[::every])
    q = 2 ** 38
    for m in (q - 1, q, q + 1):                                           # the 2^38 micro-unit limit of LD decay's sums
        b = float(Fraction(2 * m - 1, 2_000_000))                          # near (m - 1/2) / 10^6
        x += [s for s in pv.ulp_steps(b, (-2, -1, 0, 1, 2))]
    for e in (19, 32, 33, 34):                                            # prune_printed's 2^33 switch, printed_micro's 2^19
        x += pv.ulp_steps(2.0 ** e, (-2, -1, 0, 1, 2))
    x += [v * 10 ** k for v in (0.5, 0.25, 3 / 128) for k in range(0, 16)]
    return x + [-v for v in x]


def test_quantiser_is_exact(engine):
    x = _quantiser_values()
    got = engine.selftest_printed(x, precision=6, weight_type="e", min_weight=-math.inf)
    ok = checked = ties = 0
    for i, v in enumerate(x):
        want_ok = math.isfinite(v) and abs(pv.micro(v)) < 2 ** 38
        assert bool(got["micro_ok"][i]) == want_ok, (repr(v), got["micro_ok"][i])
        if want_ok:
            assert int(got["micro"][i]) == pv.micro(v), (repr(v), int(got["micro"][i]), pv.micro(v))
            ok += 1
            ties += int(pv.is_tie(np.array([v]))[0])
        checked += 1
    assert ties >= 1000
    print(f"quantiser: {checked} values, {ok} inside 2^38 micro-units equal to round_half_even(x * 10^6), {ties} exact ties")


def _label_ref(x: float, prec: int, wtype: str, min_weight: float):
    """prune_graph.pl's label of one value read back from its "%f" text: (rc, label)."""
    if not math.isfinite(x):
        return 1, 0
    w = float("%f" % x)
    if wtype == "a":
        w = abs(w)
    if w < min_weight:
        return 1, 0
    if wtype == "n":
        w = 1.0
    t = w * float(10 ** prec)
    if not -2.0 ** 62 < t < 2.0 ** 62:
        return 2, 0
    return 0, int(t)


def _labels_ref(printed: np.ndarray, prec: int, wtype: str, min_weight: float):
    """_label_ref over arrays: printed = float("%f" % x) (NaN / inf as they are)."""
    w = np.abs(printed) if wtype == "a" else printed.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        skip = ~np.isfinite(printed) | (w < min_weight)
        if wtype == "n":
            w = np.ones_like(w)
        t = w * float(10 ** prec)
        big = ~skip & ~((t > -2.0 ** 62) & (t < 2.0 ** 62))
    rc = np.where(skip, 1, np.where(big, 2, 0))
    lab = np.where(rc == 0, t, 0.0).astype(np.int64)   # (trunc toward zero: exact below 2^62)
    return rc, lab


def _host_label(x: float, prec: int, wtype: str):
    out = C.c_int64()
    rc = capi.lib().ngsld_host_prune_label(float(x), prec, wtype.encode(), C.byref(out))
    return {capi.OK: 0, capi.ERR_INVALID: 1, capi.ERR_UNSUPPORTED: 2}[rc], out.value


def test_prune_labels_equal_the_host_and_the_script(engine):
    """The device's edge labels against the script's rule on the printed text (_labels_ref) for every value, precision 0-15,
    types a / e / n; against the host's ngsld_host_prune_label (capi.prune_label's function) on every value at precisions 4
    and 6 and on every seventh value at the others."""
    x = _quantiser_values(every=64)
    printed = np.array([float("%f" % v) if math.isfinite(v) else v for v in x])
    n_ties = int(pv.is_tie(np.array(x)).sum())
    assert n_ties >= 1000
    for prec in range(16):
        for wtype in "aen":
            got = engine.selftest_printed(x, precision=prec, weight_type=wtype, min_weight=-math.inf)
            rc, lab = _labels_ref(printed, prec, wtype, -math.inf)
            g_lab = np.where(got["rc"] == 0, got["label"], 0)
            bad = np.flatnonzero((got["rc"] != rc) | (g_lab != lab))
            assert len(bad) == 0, [(repr(x[i]), prec, wtype, int(got["rc"][i]), int(got["label"][i]), int(rc[i]), int(lab[i]))
                                   for i in bad[:5]]
            for i in range(0, len(x), 1 if prec in (4, 6) else 7):   # the host's ngsld_host_prune_label: the same labels
                assert _host_label(x[i], prec, wtype) == (int(rc[i]), int(lab[i])), (repr(x[i]), prec, wtype)
    # min_weight equal to a value's printed weight: that value is an edge, the next printed weight below is not -- below the
    # 2^33 switch (a computed printed value) and above it (the value itself)
    for mw_src in (3 / 128, 0.5 + 1 / 128, 1234.5 + 1 / 128, 2.0 ** 33 + 0.5, 2.0 ** 40 + 0.25):
        mw = float("%f" % mw_src)
        xs = [mw_src] + pv.ulp_steps(mw_src) + [mw, pv.from_bits(pv.bits(mw) - 1), pv.from_bits(pv.bits(mw) + 1), mw - 1e-6,
                                                 mw + 1e-6]
        xs += [-v for v in xs]
        for prec in (4, 6):
            for wtype in "aen":
                got = engine.selftest_printed(xs, precision=prec, weight_type=wtype, min_weight=mw)
                rcs = set()
                for i, v in enumerate(xs):
                    want = _label_ref(v, prec, wtype, mw)
                    g = (int(got["rc"][i]), int(got["label"][i]) if got["rc"][i] == 0 else 0)
                    assert g == want, (repr(v), mw, prec, wtype, g, want)
                    rcs.add(want[0])
                assert rcs == {0, 1}, (mw, prec, wtype)
    print(f"prune labels: {len(x)} values ({n_ties} exact ties) x precision 0-15 x types a/e/n equal to host and script")
