"""div_nearest (ngsld_amd/csrc/ld_mean.h) -- the one rounding behind every mean of ngsld_decay and ngsld_site_ld -- held to the
exact quotient: it must give float(Fraction(a, b)), which rounds half to even, on exact ties, their neighbours, means of
micro-unit sums and operands beyond 64 bits.  No GPU: the header is plain C++ and is compiled alone."""
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
    const double v = ngsld::eng::div_nearest(x, y);
    uint64_t w;
    std::memcpy(&w, &v, 8);
    std::printf("%016llx\n", (unsigned long long)w);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("div_nearest")
    (d / "h.cpp").write_text(HARNESS)
    exe = str(d / "h")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(capi.PKG_DIR, "csrc"), "-o", exe,
                           str(d / "h.cpp")])
    return exe


def _operands():
    rng = random.Random(20240611)
    ops = [(0, 7), (1, 1), (1, 3), (2, 3), (300001, 3000000), (1, 10 ** 6), (2 ** 38 - 1, 1), ((2 ** 38 - 1) * 5, 5 * 10 ** 6)]
    # exact ties at the 54th bit and their neighbours: a / b = (2 m + 1) / 2^k with a 53-bit m, one unit either side
    for _ in range(4000):
        m = rng.getrandbits(52) | (1 << 52)
        k = rng.randrange(54, 62)
        b = 1 << k
        scale = rng.choice([1, 3, 5, 10 ** 6])
        for da in (-1, 0, 1):
            ops.append(((2 * m + 1) * scale + da, b * scale >> 0))
    # means of micro-unit sums: n rows, |q| < 2^38
    for _ in range(20000):
        n = rng.choice([1, 2, 3, 7, rng.randrange(1, 2000), rng.randrange(1, 1 << rng.randrange(1, 34))])
        s = rng.randrange(0, min(n * (2 ** 38 - 1), 2 ** 63 - 1) + 1) >> rng.randrange(0, 40)
        ops.append((s, n * 10 ** 6))
    # operands beyond 64 bits (decay's 128-bit totals)
    for _ in range(4000):
        b = rng.getrandbits(rng.randrange(64, 100)) | (1 << 63)
        a = (b * rng.getrandbits(rng.randrange(1, 54))) >> rng.randrange(0, 30)
        ops.append((a, b))
    return [(a, b) for a, b in ops if b > 0 and a // b < 2 ** 54 and b < 2 ** 126 and a < 2 ** 128]  # (the function's domain)


def test_div_nearest_gives_the_exact_quotient_rounded_once(harness):
    ops = _operands()
    text = "".join(f"{a} {b}\n" for a, b in ops)
    out = subprocess.run([harness], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(ops) + 1 and len(ops) > 30000
    for (a, b), line in zip(ops, out):
        got = struct.unpack(">d", bytes.fromhex(line))[0]
        assert got.hex() == float(Fraction(a, b)).hex(), (a, b, got)
