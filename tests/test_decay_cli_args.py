"""The binary's --decay_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid decay command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("decay_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


LD_MSG = "--decay_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
BAD = [
    (["--decay_out", "b", "--decay_ld", "r3"], LD_MSG),
    (["--decay_out", "b", "--decay_ld", "r2,"], LD_MSG),
    (["--decay_out", "b", "--decay_ld", ""], LD_MSG),
    (["--decay_out", "b", "--decay_ld", "r2 Dp"], LD_MSG),
    (["--decay_out", "b", "--decay_bin_size", "1"], "--decay_bin_size must be a number > 1!"),
    (["--decay_out", "b", "--decay_bin_size", "0.5"], "--decay_bin_size must be a number > 1!"),
    (["--decay_out", "b", "--decay_bin_size", "inf"], "--decay_bin_size must be a number > 1!"),
    (["--decay_out", "b", "--decay_bin_size", "nan"], "--decay_bin_size must be a number > 1!"),
    (["--decay_out", "b", "--decay_bin_size", "250bp"], "--decay_bin_size must be a number > 1!"),
    (["--decay_out", "b", "--decay_max_kb_dist", "-1"], "--decay_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--decay_out", "b", "--decay_max_kb_dist", "nan"], "--decay_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--decay_out", "b", "--decay_max_kb_dist", "x"], "--decay_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--decay_out", "b", "--decay_min_maf", "-0.1"], "--decay_min_maf must be a number >= 0!"),
    (["--decay_out", "b", "--decay_min_maf", "inf"], "--decay_min_maf must be a number >= 0!"),
    (["--decay_out", "b", "--decay_min_maf", ""], "--decay_min_maf must be a number >= 0!"),
    (["--decay_out", "b", "--decay_n_ind", "-5"], "--decay_n_ind must be a number >= 0!"),
    (["--decay_out", "b", "--decay_n_ind", "ten"], "--decay_n_ind must be a number >= 0!"),
    (["--decay_out", "b", "--decay_recomb_rate", "0"], "--decay_recomb_rate must be a number > 0!"),
    (["--decay_out", "b", "--decay_recomb_rate", "-1"], "--decay_recomb_rate must be a number > 0!"),
    (["--decay_out", "b", "--decay_recomb_rate", "inf"], "--decay_recomb_rate must be a number > 0!"),
    (["--decay_out", "b", "--decay_n_ind", "20", "--decay_ld", "D,Dp"], "--decay_n_ind is only used for the r2 and r2_ExpG fits!"),
    (["--decay_fit", "f", "--decay_n_ind", "20", "--decay_ld", "r2,Dp"], "--decay_n_ind cannot be combined with a Dp fit!"),
    (["--decay_out", "b", "--devices", "0-1"], "--decay_out runs on one device: it cannot be combined with --devices!"),
    (["--decay_fit", "f", "--devices", "0,0"], "--decay_out runs on one device: it cannot be combined with --devices!"),
    (["--decay_ld", "r2"], "the --decay_* options need --decay_out FILE or --decay_fit FILE!"),
    (["--decay_bin_size", "100"], "the --decay_* options need --decay_out FILE or --decay_fit FILE!"),
    (["--decay_out="], "--decay_out needs a file name!"),
    (["--decay_out", "b", "--decay_fit="], "--decay_fit needs a file name!"),
    (["--decay_out", "b", "--decay_what", "1"], "unknown option --decay_what!"),
    (["--decay_out", "b", "--decay_bin_size"], "--decay_bin_size needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--decay_out", "b", "--decay_max_kb_dist=-1"], "--decay_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--decay_out", "b", "-decay_max_kb_dist", "-1"], "--decay_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--decay_min_maf", "0.1", "--", "--decay_out", "b"], "the --decay_* options need --decay_out FILE or --decay_fit FILE!"),
    (["--decay_out", "b", "--decay_zzz"], "unknown option --decay_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_decay_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "b") and not os.path.exists(inputs / "f")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--decay_out", "b"],
    ["-decay_out", "b", "--decay_fit", "f", "--decay_ld", "r2_ExpG,D,Dp,r2", "--decay_bin_size=62.5", "--decay_max_kb_dist",
     "inf", "--decay_min_maf", "0.05", "--decay_recomb_rate", "0.5"],
    ["--decay_fit=f", "--decay_n_ind", "40", "--decay_ld", "r2", "--out", "t.tsv", "--prune_out", "k"],
])
def test_valid_decay_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
def test_prefixes_of_the_reference_flags_are_unchanged(inputs):
    """The --decay_* flags are exact names taken out of argv before getopt: the reference's own abbreviations still work
    beside them ("--n_thr" is --n_threads), and "--de" is still ambiguous among its --device / --devices."""
    r = _run(inputs, "--decay_out", "b", "--n_thr", "2", "--verbose", "1")
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
    r = _run(inputs, "--de", "0")
    assert "is ambiguous" in r.stderr and "decay" not in r.stderr
