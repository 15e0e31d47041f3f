"""mean_nearest (ngsld_amd/csrc/ld_mean.h) -- the mean of ngsld_grid's cells -- held to the exact quotient on both of its
branches: one IEEE division where the sum is below 2^53 and the rows below 2^33, div_nearest's long division elsewhere.  It must
give float(Fraction(sum, 10^6 * rows)) on either side of both thresholds.  No GPU: the header is plain C++ and is compiled alone."""
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
int main() {
  unsigned long long a, b;
  while (std::scanf("%llu %llu", &a, &b) == 2) {
    const double v = ngsld::eng::mean_nearest(a, b);
    uint64_t w;
    std::memcpy(&w, &v, 8);
    std::printf("%016llx\n", (unsigned long long)w);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("mean_nearest")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(capi.PKG_DIR, "csrc"), "-o", exe,
                           str(d / "h.cpp")])
    return exe


def _operands():
    rng = random.Random(20261018)
    ops = [(0, 1), (0, 7), (1, 1), (300001, 3), (250000, 1), (2 ** 38 - 1, 1), (2 ** 53 - 1, 1), (2 ** 53, 1), (2 ** 53 + 1, 3),
           (2 ** 53 - 1, 2 ** 33 - 1), (2 ** 53 - 1, 2 ** 33), (5, 2 ** 33), (2 ** 63 - 1, 2 ** 25), (2 ** 63 - 1, 2 ** 40)]
    # cells as the grid makes them: n rows of |q| < 2^38 (a sum below 2^53 up to 2^15 rows of the largest value)
    for _ in range(20000):
        n = rng.choice([1, 2, 3, 7, rng.randrange(1, 2000), rng.randrange(1, 1 << rng.randrange(1, 26))])
        s = rng.randrange(0, min(n * (2 ** 38 - 1), 2 ** 63 - 1) + 1) >> rng.randrange(0, 40)
        ops.append((s, n))
    # either side of the sum's threshold, at row counts whose denominators share every factor of 10^6 with them or none
    for _ in range(4000):
        s = 2 ** 53 + rng.randrange(-2000, 2000)
        ops.append((s, rng.choice([1, 3, 2 ** 15, 5 ** 6, 2 ** 33 - 1, 2 ** 33, rng.randrange(2 ** 15, 2 ** 34)])))
    # quotients one unit either side of a 54-bit tie of the long branch: sum = (2 m + 1) * 5^6 * r + d over rows = 2^k * r
    for _ in range(4000):
        m = rng.getrandbits(40) | (1 << 40)
        k, r = rng.randrange(0, 12), rng.choice([1, 3, 7])
        for d in (-1, 0, 1):
            ops.append(((2 * m + 1) * 5 ** 6 * r + d, (1 << k) * r))
    return [(s, n) for s, n in ops if 0 <= s < 2 ** 63 and 0 < n < 2 ** 44 and s // (n * 10 ** 6) < 2 ** 54]


def test_mean_nearest_gives_the_exact_mean_rounded_once_on_both_branches(harness):
    ops = _operands()
    short = sum(1 for s, n in ops if s < 2 ** 53 and n < 2 ** 33)
    assert short > 20000 and len(ops) - short > 1500  # (both branches are run)
    text = "".join(f"{s} {n}\n" for s, n in ops)
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(ops) + 1
    for (s, n), line in zip(ops, out):
        got = struct.unpack(">d", bytes.fromhex(line))[0]
        assert got.hex() == float(Fraction(s, n * 10 ** 6)).hex(), (s, n, got)
