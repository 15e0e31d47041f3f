"""The binary's --site_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid site command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("site_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


LD_MSG = "--site_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
NEED_OUT = "the --site_* options need --site_out FILE!"
BAD = [
    (["--site_out", "s", "--site_ld", "r3"], LD_MSG),
    (["--site_out", "s", "--site_ld", "r2,"], LD_MSG),
    (["--site_out", "s", "--site_ld", ""], LD_MSG),
    (["--site_out", "s", "--site_ld", "r2 Dp"], LD_MSG),
    (["--site_out", "s", "--site_max_kb_dist", "-1"], "--site_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--site_out", "s", "--site_max_kb_dist", "nan"], "--site_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--site_out", "s", "--site_max_kb_dist", "10kb"], "--site_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--site_out", "s", "--site_min_maf", "-0.1"], "--site_min_maf must be a number >= 0!"),
    (["--site_out", "s", "--site_min_maf", "inf"], "--site_min_maf must be a number >= 0!"),
    (["--site_out", "s", "--site_min_maf", ""], "--site_min_maf must be a number >= 0!"),
    (["--site_out", "s", "--site_linked_min", "nan"], "--site_linked_min must be a number!"),
    (["--site_out", "s", "--site_linked_min", "half"], "--site_linked_min must be a number!"),
    (["--site_out", "s", "--site_linked_min="], "--site_linked_min must be a number!"),
    (["--site_out", "s", "--devices", "0-1"], "--site_out runs on one device: it cannot be combined with --devices!"),
    (["--site_out", "s", "--site_signed", "--devices", "0,0"], "--site_out runs on one device: it cannot be combined with --devices!"),
    (["--site_ld", "r2"], NEED_OUT),
    (["--site_signed"], NEED_OUT),
    (["--site_linked_min", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--site_out="], "--site_out needs a file name!"),
    (["--site_out", "s", "--site_what", "1"], "unknown option --site_what!"),
    (["--site_out", "s", "--site_signed=1"], "unknown option --site_signed!"),
    (["--site_out", "s", "--site_min_maf"], "--site_min_maf needs a value!"),
    (["--site_out"], "--site_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--site_out", "s", "--site_min_maf=-0.1"], "--site_min_maf must be a number >= 0!"),
    (["--site_out", "s", "-site_min_maf", "-0.1"], "--site_min_maf must be a number >= 0!"),
    (["--site_min_maf", "0.1", "--", "--site_out", "s"], "the --site_* options need --site_out FILE!"),
    (["--site_out", "s", "--site_zzz"], "unknown option --site_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_site_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t.tsv")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--site_out", "s"],
    ["-site_out", "s", "--site_ld", "r2_ExpG,D,Dp,r2", "--site_max_kb_dist=inf", "--site_min_maf", "0.05", "--site_linked_min",
     "-0.2", "--site_signed"],
    ["--site_out=s", "--site_ld", "Dp", "--out", "t.tsv", "--prune_out", "k", "--decay_out", "b"],
])
def test_valid_site_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(inputs / "s")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
def test_prefixes_of_the_reference_flags_are_unchanged(inputs):
    """The --site_* flags are exact names taken out of argv before getopt: the reference's own abbreviations still work beside
    them ("--n_thr" is --n_threads, "--n_s" --n_sites), with and without --pos."""
    r = _run(inputs, "--site_out", "s", "--n_thr", "2", "--verbose", "1")
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
    argv = [capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_s", "10", "--max_kb_dist", "0", "--site_out", "s"]
    r = subprocess.run(argv, capture_output=True, text=True, cwd=str(inputs), timeout=120)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
