"""The binary's --scan_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid scan command line gets as far as the device.  (Whether a matrix is cut into
slabs is decided from the device's memory: that refusal is in tests/test_gpu_scan.py, with the binary's other runs.)"""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("scan_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


OK = ["--scan_out", "s", "--scan_half_window", "100"]
LD_MSG = "--scan_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
NEED_OUT = "the --scan_* options need --scan_out FILE!"
NEED_H = "--scan_out needs the half window in bp: --scan_half_window INT!"
BAD_H = "--scan_half_window must be an integer in [0, 2147483647]!"
ONE_DEVICE = "--scan_out runs on one device: it cannot be combined with --devices!"
BAD = [
    (["--scan_out", "s"], NEED_H),
    (["--scan_out", "s", "--scan_ld", "r2"], NEED_H),
    (["--scan_out", "s", "--scan_half_window", "-1"], BAD_H),
    (["--scan_out", "s", "--scan_half_window", "1.5"], BAD_H),
    (["--scan_out", "s", "--scan_half_window", "5kb"], BAD_H),
    (["--scan_out", "s", "--scan_half_window", ""], BAD_H),
    (["--scan_out", "s", "--scan_half_window", "inf"], BAD_H),
    (["--scan_out", "s", "--scan_half_window", "2147483648"], BAD_H),
    (["--scan_out", "s", "--scan_half_window", "99999999999999999999"], BAD_H),
    ([*OK, "--scan_ld", "r3"], LD_MSG),
    ([*OK, "--scan_ld", "r2,"], LD_MSG),
    ([*OK, "--scan_ld", ""], LD_MSG),
    ([*OK, "--scan_ld", "r2 Dp"], LD_MSG),
    ([*OK, "--scan_max_kb_dist", "-1"], "--scan_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*OK, "--scan_max_kb_dist", "nan"], "--scan_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*OK, "--scan_max_kb_dist", "10kb"], "--scan_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*OK, "--scan_min_maf", "-0.1"], "--scan_min_maf must be a number >= 0!"),
    ([*OK, "--scan_min_maf", "inf"], "--scan_min_maf must be a number >= 0!"),
    ([*OK, "--scan_min_maf", ""], "--scan_min_maf must be a number >= 0!"),
    # a window wider than the table's: the plan holds the pairs up to 100 kb apart (the reference's default), 7 kb here
    (["--scan_out", "s", "--scan_half_window", "50001"], "needs the pairs up to 100002 bp apart: --max_kb_dist holds them up to 100000 bp!"),
    (["--scan_out", "s", "--scan_half_window", "3501", "--max_kb_dist", "7"],
     "--scan_half_window 3501 needs the pairs up to 7002 bp apart: --max_kb_dist holds them up to 7000 bp!"),
    ([*OK, "--devices", "0-1"], ONE_DEVICE),
    ([*OK, "--scan_min_maf", "0.1", "--devices", "0,0"], ONE_DEVICE),
    (["--scan_ld", "r2"], NEED_OUT),
    (["--scan_half_window", "100"], NEED_OUT),
    (["--scan_min_maf", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--scan_out=", "--scan_half_window", "100"], "--scan_out needs a file name!"),
    ([*OK, "--scan_what", "1"], "unknown option --scan_what!"),
    ([*OK, "--scan_signed"], "unknown option --scan_signed!"),
    ([*OK, "--scan_min_maf"], "--scan_min_maf needs a value!"),
    (["--scan_out"], "--scan_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    ([*OK, "--scan_min_maf=-0.1"], "--scan_min_maf must be a number >= 0!"),
    ([*OK, "-scan_min_maf", "-0.1"], "--scan_min_maf must be a number >= 0!"),
    (["--scan_half_window=100", "--", "--scan_out", "s"], NEED_OUT),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_scan_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t.tsv")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    OK,
    ["-scan_out", "s", "--scan_half_window=0", "--scan_ld", "r2_ExpG,D,Dp,r2", "--scan_max_kb_dist=inf", "--scan_min_maf", "0.05"],
    ["--scan_out=s", "--scan_half_window", "50000", "--scan_ld", "Dp", "--out", "t.tsv", "--site_out", "k", "--decay_out", "b"],
    ["--scan_out", "s", "--scan_half_window", "2147483647", "--max_kb_dist", "0"],  # (all pairs: any half window)
    ["--scan_out", "s", "--scan_half_window", "3500", "--max_kb_dist", "7"],
])
def test_valid_scan_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(inputs / "s")
