"""div_nearest_small (ngsld_amd/csrc/ld_mean.h) -- the means of ngsld_decay_map's bins: the hardware quotient where both operands
are below 2^53, div_nearest otherwise -- held to the exact quotient, float(Fraction(a, b)), on both sides of 2^53: exact ties at
the 54th bit and their neighbours, means of micro-unit sums, and the operands at the threshold.  No GPU: the header is plain C++
and is compiled alone, with the product's -ffp-contract=off."""
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
    const double v = ngsld::eng::div_nearest_small(read_u128(a), read_u128(b));
    uint64_t w;
    std::memcpy(&w, &v, 8);
    std::printf("%016llx\n", (unsigned long long)w);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("div_nearest_small")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(capi.PKG_DIR, "csrc"), "-o", exe,
                           str(d / "h.cpp")])
    return exe


def _operands():
    rng = random.Random(20261021)
    T = 2 ** 53
    ops = [(0, 7), (1, 1), (1, 3), (2, 3), (300001, 3000000), (1, 10 ** 6), (2 ** 38 - 1, 10 ** 6)]
    # the threshold itself: each operand just below, at and above 2^53
    for a in (T - 2, T - 1, T, T + 1):
        for b in (1, 3, 10 ** 6, T - 1, T, T + 1):
            ops.append((a, b))
    # exact ties at the 54th bit and their neighbours with both operands below 2^53: (2 m + 1) / 2^k needs a 53-bit result from
    # a numerator below 2^53, so m has fewer bits and the tie lies in a shorter quotient -- and ties of full length beside them,
    # which div_nearest takes
    for _ in range(6000):
        bits = rng.randrange(2, 52)
        m = rng.getrandbits(bits) | (1 << bits)
        k = rng.randrange(1, 52)
        for da in (-1, 0, 1):
            ops.append((2 * m + 1 + da, 1 << k))
        m = rng.getrandbits(52) | (1 << 52)
        ops.append((2 * m + 1, 1 << rng.randrange(54, 62)))
    # quotients that need more than 53 bits: a / b with b odd never ends, a * 2^j / (b * 2^j) the same
    for _ in range(6000):
        b = rng.randrange(3, 2 ** rng.randrange(3, 53)) | 1
        a = rng.randrange(1, T)
        ops.append((a, b))
    # means of micro-unit sums: n rows, |q| < 2^38, on either side of the threshold
    for _ in range(20000):
        n = rng.choice([1, 2, 3, 7, rng.randrange(1, 2000), rng.randrange(1, 1 << rng.randrange(1, 34))])
        s = rng.randrange(0, min(n * (2 ** 38 - 1), 2 ** 63 - 1) + 1) >> rng.randrange(0, 40)
        ops.append((s, n * 10 ** 6))
    return [(a, b) for a, b in ops if b > 0 and a // b < 2 ** 54]  # (div_nearest's domain)


def test_div_nearest_small_gives_the_exact_quotient_rounded_once(harness):
    ops = _operands()
    small = sum(1 for a, b in ops if a < 2 ** 53 and b < 2 ** 53)
    assert small > 20000 and len(ops) - small > 5000  # (both paths)
    text = "".join(f"{a} {b}\n" for a, b in ops)
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(ops) + 1
    for (a, b), line in zip(ops, out):
        got = struct.unpack(">d", bytes.fromhex(line))[0]
        assert got.hex() == float(Fraction(a, b)).hex(), (a, b, got)
