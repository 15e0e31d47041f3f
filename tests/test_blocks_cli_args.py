"""The binary's --blocks_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid blocks command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("blocks_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra, pos=True):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10",
            *(["--pos", str(d / "p.pos")] if pos else []), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


REGION = ["--blocks_chr", "1", "--blocks_start", "1", "--blocks_end", "50"]
LD_MSG = "--blocks_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
BAD = [
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "50", "--blocks_end", "50"],
     "start position must be smaller than end position."),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "60", "--blocks_end", "50"],
     "start position must be smaller than end position."),
    (["--blocks_out", "b", "--blocks_start", "1", "--blocks_end", "50"], "--blocks_out needs the region's chromosome: --blocks_chr CHR!"),
    (["--blocks_out", "b", "--blocks_chr=", "--blocks_start", "1", "--blocks_end", "50"],
     "--blocks_out needs the region's chromosome: --blocks_chr CHR!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_end", "50"], "--blocks_out needs the region's start: --blocks_start INT!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "1"], "--blocks_out needs the region's end: --blocks_end INT!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "-1", "--blocks_end", "50"],
     "--blocks_start must be a non-negative integer!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "1.5", "--blocks_end", "50"],
     "--blocks_start must be a non-negative integer!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "1", "--blocks_end", "5e3"],
     "--blocks_end must be a non-negative integer!"),
    (["--blocks_out", "b", "--blocks_chr", "1", "--blocks_start", "1", "--blocks_end", ""], "--blocks_end must be a non-negative integer!"),
    (["--blocks_out", "b", *REGION, "--blocks_ld", "r3"], LD_MSG),
    (["--blocks_out", "b", *REGION, "--blocks_ld", "r2,"], LD_MSG),
    (["--blocks_out", "b", *REGION, "--blocks_ld", ""], LD_MSG),
    (["--blocks_out", "b", *REGION, "--blocks_ld", "r2 Dp"], LD_MSG),
    (["--blocks_out", "b", *REGION, "--devices", "0-1"], "--blocks_out runs on one device: it cannot be combined with --devices!"),
    ([*REGION], "the --blocks_* options need --blocks_out PREFIX!"),
    (["--blocks_ld", "r2"], "the --blocks_* options need --blocks_out PREFIX!"),
    (["--blocks_out=", *REGION], "--blocks_out needs a file name prefix!"),
    (["--blocks_out", "b", *REGION, "--blocks_what", "1"], "unknown option --blocks_what!"),
    (["--blocks_out", "b", "--blocks_chr"], "--blocks_chr needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--blocks_out", "b", *REGION, "--blocks_ld=r3"], "--blocks_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"),
    (["--blocks_out", "b", *REGION, "-blocks_ld", "r3"], "--blocks_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"),
    ([*REGION, "--", "--blocks_out", "b"], "the --blocks_* options need --blocks_out PREFIX!"),
    (["--blocks_out", "b", *REGION, "--blocks_zzz"], "unknown option --blocks_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_blocks_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not any(name.startswith("b.") for name in os.listdir(inputs))


def test_blocks_need_positions(inputs):
    r = _run(inputs, "--blocks_out", "b", *REGION, "--max_kb_dist", "0", pos=False)  # (a distance limit needs --pos too)
    assert r.returncode == 255 and "--blocks_out needs positions: it cannot run without --pos!" in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--blocks_out", "b", *REGION],
    ["-blocks_out", "b", "--blocks_chr=1", "--blocks_start=0", "--blocks_end=9999999999999999999", "--blocks_ld",
     "r2_ExpG,D,Dp,r2"],
    ["--blocks_out=b", *REGION, "--out", "t.tsv", "--prune_out", "k", "--decay_out", "d"],
])
def test_valid_blocks_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
def test_prefixes_of_the_reference_flags_are_unchanged(inputs):
    """The --blocks_* flags are exact names taken out of argv before getopt: the reference's own abbreviations still work."""
    r = _run(inputs, "--blocks_out", "b", *REGION, "--n_thr", "2", "--verbose", "1")
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
