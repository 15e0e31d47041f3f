"""Doubles where a "%f" formatter goes wrong, shared by the host formatter's test (test_host_io.py) and the device's
(test_gpu_printed_values.py), with the exact reference of what they print: Python's % formatting rounds the exact binary value
half-to-even, as glibc does."""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b) & (2 ** 64 - 1)))[0]


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def host_format_values() -> list[float]:
    """The values test_format_double_is_printf_exact has always held the host formatter to (the same ones, in the same
    order): magnitudes, ties, subnormals and bit patterns of every kind (NaN among them)."""
    rng = np.random.default_rng(11)
    vals = [0.0, -0.0, 1.0, -1.0, 0.5, 0.0078125, 0.00390625, 2.5e-7, 5e-7, 4.9999999999999998e-7, 1.5e-6, 0.1, 0.7,
            1e-300, 5e-324, 123456789.987654321, 9.2e12, 9.3e12, 1e15, 2.0 ** 53, 2.0 ** 63, 1e22, 1e300,
            999999.9999995, 0.9999995, 0.9999994999999999, 1 - 2.0 ** -53]
    vals += list(rng.random(60000))                                        # [0,1): the bulk of what is printed
    vals += list((rng.random(60000) - 0.5) * 10.0 ** rng.integers(-12, 14, 60000))
    vals += [from_bits(b) for b in rng.integers(0, 2 ** 63, 40000)]
    # exact ties at the 6th decimal: k / 2^j with 7+ decimals
    vals += [float(k) / 2.0 ** j for j in range(7, 20) for k in range(1, 200, 2)]
    return vals


def ulp_steps(x: float, steps=(-2, -1, 1, 2)) -> list[float]:
    """x moved by whole ulps (the bit pattern of a finite positive x plus k)."""
    return [from_bits(bits(x) + k) for k in steps]


def odd_128_ties(limit: float = 4.0) -> list[float]:
    """Every x = odd / 128 in (0, limit): exactly the doubles of that range whose x * 10^6 ends in .5 (the only dyadic
    rationals with a tie at the sixth decimal), what called genotypes of small cohorts give D."""
    return [k / 128.0 for k in range(1, int(limit * 128), 2)]


def tie_values() -> list[float]:
    """Ties at the sixth decimal, their neighbours at +-1 and +-2 ulp, and all of them negated."""
    out = []
    for t in odd_128_ties(8.0) + [float(k) / 2.0 ** 7 for k in (12_800_001, 127_999_999)]:   # (and two near 10^5 and 10^6)
        out += [t] + ulp_steps(t)
    return out + [-x for x in out]


def negative_zero_values() -> list[float]:
    """Values that print "-0.000000": -0.0 and negatives up to the tie at -5e-7 (which rounds to even: to zero)."""
    half = 5e-7 if Fraction(5e-7) < Fraction(1, 2_000_000) else from_bits(bits(5e-7) - 1)   # largest double below 5e-7
    return [-0.0, -5e-324, -1e-300, -2.0 ** -1022, -1e-7, -4e-7, -half, -2.0 ** -21, -from_bits(bits(2.0 ** -21) - 1)]


def subnormal_values() -> list[float]:
    return [5e-324, 1e-320, 2.0 ** -1060, from_bits(0x000fffffffffffff), 2.0 ** -1022, from_bits(0x0010000000000001)]


def limit_values() -> list[float]:
    """Around the device formatter's fast path (a quotient of 63 bits: |v| * 10^6 < 2^63 for "%f") and the 2^52 / 2^53 limits."""
    out = [2.0 ** 52, 2.0 ** 53, 9.2e12, 9.3e12, 2.0 ** 63 / 1e6]
    out += ulp_steps(2.0 ** 52, (-1, 1)) + ulp_steps(2.0 ** 53, (-1, 1)) + ulp_steps(2.0 ** 63 / 1e6, (-2, -1, 1, 2))
    return out + [-x for x in out]


def nonfinite_values() -> list[float]:
    return [float("nan"), -float("nan"), from_bits(0x7ff0000000000001), from_bits(0xfff8000000000001), float("inf"),
            -float("inf")]


def printf_f(v: float) -> str:
    """What glibc's "%f" prints for v (NaN of either sign as "-nan", the reference's build)."""
    return "-nan" if v != v else "%f" % v


def needs_host(v: float) -> bool:
    """Whether v lies beyond the device formatter's "%f" fast path: floor(|v| * 10^6) >= 2^63 (so from ~9.22e12 on, 2^52
    included).  Such a batch goes to the host as records."""
    return v == v and abs(v) != float("inf") and int(Fraction(abs(v)) * 10 ** 6) >= 2 ** 63


def round_half_even(f: Fraction) -> int:
    """The integer nearest to f, ties to even."""
    q, r = divmod(f.numerator, f.denominator)
    if 2 * r > f.denominator or (2 * r == f.denominator and q % 2):
        q += 1
    return q


def micro(x: float) -> int:
    """round_half_even(x * 10^6): the digits of "%f" % x without the point, signed."""
    m = round_half_even(abs(Fraction(x)) * 10 ** 6)
    return -m if x < 0 else m


def is_tie(x: np.ndarray) -> np.ndarray:
    """Element-wise: x * 10^6 ends in exactly .5, i.e. x * 128 is an odd integer (x * 128 is exact)."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.asarray(x, dtype=np.float64) * 128.0
        return np.isfinite(y) & (np.abs(y) < 2.0 ** 53) & (np.floor(y) == y) & (np.fmod(y, 2.0) != 0)
