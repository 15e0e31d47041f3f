"""ratio_nearest (ngsld_amd/csrc/ld_mean.h) -- the one rounding behind ngsld_scan's omega -- held to the exact quotient: it must
give float(Fraction(num, den)), which rounds half to even, on exact ties, their neighbours, quotients below 2^-60 and above
2^70, operands on both sides of the 2^53 threshold of its short path, and products of sums and counts as the scan forms them.
No GPU: the header is plain C++ and is compiled alone, as tests/test_div_nearest.py does."""
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

from ngsld_amd import capi

HARNESS = r"""
#include <cstdio>
#include <cstring>
#include "ld_mean.h"
static unsigned __int128 read_u128(const char *s) {
  unsigned __int128 v = 0;
  for (; *s >= '0' && *s <= '9'; ++s) v = v * 10 + (unsigned)(*s - '0');
  return v;
}
int main() {
  char a[64], b[64];
  while (std::scanf("%63s %63s", a, b) == 2) {
    const unsigned __int128 x = read_u128(a), y = read_u128(b);
    const double v = ngsld::eng::ratio_nearest(x, y);
    uint64_t w;
    std::memcpy(&w, &v, 8);
    std::printf("%016llx\n", (unsigned long long)w);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("ratio_nearest")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(capi.PKG_DIR, "csrc"), "-o", exe,
                           str(d / "h.cpp")])
    return exe


def _run(harness, ops):
    assert all(0 <= a < 2 ** 128 and 0 < b < 2 ** 127 for a, b in ops)  # (the function's domain)
    text = "".join(f"{a} {b}\n" for a, b in ops)
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(ops) + 1
    for (a, b), line in zip(ops, out):
        got = struct.unpack(">d", bytes.fromhex(line))[0]
        assert got.hex() == float(Fraction(a, b)).hex(), (a, b, got)


def test_small_cases_and_the_short_path_threshold(harness):
    T = 2 ** 53
    ops = [(0, 7), (0, 2 ** 100), (1, 1), (1, 3), (2, 3), (10, 4), (1, 2 ** 126), (2 ** 128 - 1, 1), (2 ** 128 - 1, 2 ** 127 - 1),
           (2 ** 128 - 1, 3), (1, 2 ** 127 - 1)]
    # both sides of 2^53 in either operand: the last pair of doubles, the first of the long division
    for a in (T - 2, T - 1, T, T + 1, T + 2):
        for b in (1, 3, 7, 10 ** 6, T - 2, T - 1, T, T + 1, T + 2, 3 * T + 1):
            ops += [(a, b), (b, a)]
    rng = random.Random(53)
    for _ in range(4000):
        a, b = rng.randrange(T - 4096, T + 4096), rng.randrange(1, T + 4096)
        ops += [(a, b), (b, a)]
    _run(harness, ops)


def test_ties_and_their_neighbours(harness):
    """num / den = (2 m + 1) * 2^k with a 53-bit m: an exact tie between two doubles, and one unit of num either side; k from
    far below to far above 1, the operands scaled by odd numbers so that the tie is not visible in either alone."""
    rng = random.Random(20250611)
    ops = []
    for _ in range(6000):
        m = rng.getrandbits(52) | (1 << 52)
        k = rng.randrange(-70, 70)
        scale = rng.choice([1, 3, 5, 10 ** 6 + 1, rng.getrandbits(30) | 1])
        num, den = ((2 * m + 1) << max(k, 0)) * scale, (1 << max(-k, 0)) * scale
        if num + 1 >= 2 ** 128 or den >= 2 ** 127:
            continue
        for da in (-1, 0, 1):
            ops.append((num + da, den))
    assert len(ops) > 15000
    _run(harness, ops)


def test_tiny_and_huge_quotients(harness):
    rng = random.Random(7)
    ops = []
    for _ in range(6000):
        small = rng.getrandbits(rng.randrange(1, 60)) | 1
        big = rng.getrandbits(rng.randrange(62, 127)) | (1 << 61)
        ops += [(small, big), (big, small)]
    below = [Fraction(a, b) for a, b in ops if Fraction(a, b) < Fraction(1, 2 ** 60)]
    above = [Fraction(a, b) for a, b in ops if Fraction(a, b) > 2 ** 70]
    assert len(below) > 500 and len(above) > 500
    _run(harness, ops)


def test_products_of_sums_and_counts(harness):
    """omega's operands: (S_LL + S_RR) * n_LR over (n_LL + n_RR) * S_LR with sums below 2^63 and counts below 2^63."""
    rng = random.Random(11)
    ops = []
    for _ in range(20000):
        n_in, n_lr = rng.randrange(1, 1 << rng.randrange(1, 63)), rng.randrange(1, 1 << rng.randrange(1, 63))
        s_in, s_lr = rng.randrange(0, 1 << rng.randrange(1, 63)), rng.randrange(1, 1 << rng.randrange(1, 63))
        ops.append((s_in * n_lr, n_in * s_lr))
    _run(harness, ops)
