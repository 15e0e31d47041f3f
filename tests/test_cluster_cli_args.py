"""The binary's --cluster_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid cluster command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("cluster_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


FIELD_MSG = "--cluster_field must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!"
NEED_OUT = "the --cluster_* options need --cluster_out FILE or --cluster_table FILE!"
KB_MSG = "--cluster_max_kb_dist must be a number >= 0 (or inf)!"
MAF_MSG = "--cluster_min_maf must be a number >= 0!"
SIZE_MSG = "--cluster_min_size must be an integer >= 1!"
DEV_MSG = "--cluster_out runs on one device: it cannot be combined with --devices!"
BAD = [
    (["--cluster_out", "s", "--cluster_field", "3"], FIELD_MSG),
    (["--cluster_out", "s", "--cluster_field", "8"], FIELD_MSG),
    (["--cluster_out", "s", "--cluster_field", "r2"], FIELD_MSG),
    (["--cluster_table", "t", "--cluster_field", ""], FIELD_MSG),
    (["--cluster_out", "s", "--cluster_field", "7.0"], FIELD_MSG),
    (["--cluster_out", "s", "--cluster_min_weight", "nan"], "--cluster_min_weight must be a number!"),
    (["--cluster_out", "s", "--cluster_min_weight", "half"], "--cluster_min_weight must be a number!"),
    (["--cluster_table", "t", "--cluster_min_weight="], "--cluster_min_weight must be a number!"),
    (["--cluster_out", "s", "--cluster_max_kb_dist", "-1"], KB_MSG),
    (["--cluster_out", "s", "--cluster_max_kb_dist", "nan"], KB_MSG),
    (["--cluster_out", "s", "--cluster_max_kb_dist", "10kb"], KB_MSG),
    (["--cluster_out", "s", "--cluster_min_maf", "-0.1"], MAF_MSG),
    (["--cluster_out", "s", "--cluster_min_maf", "inf"], MAF_MSG),
    (["--cluster_out", "s", "--cluster_min_maf", ""], MAF_MSG),
    (["--cluster_table", "t", "--cluster_min_size", "0"], SIZE_MSG),
    (["--cluster_table", "t", "--cluster_min_size", "-2"], SIZE_MSG),
    (["--cluster_table", "t", "--cluster_min_size", "2.5"], SIZE_MSG),
    (["--cluster_table", "t", "--cluster_min_size", "two"], SIZE_MSG),
    (["--cluster_table", "t", "--cluster_min_size", "99999999999"], SIZE_MSG),
    (["--cluster_out", "s", "--devices", "0-1"], DEV_MSG),
    (["--cluster_table", "t", "--cluster_signed", "--devices", "0,0"], DEV_MSG),
    (["--cluster_field", "7"], NEED_OUT),
    (["--cluster_signed"], NEED_OUT),
    (["--cluster_min_weight", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--cluster_min_size", "3", "--site_out", "s"], NEED_OUT),
    (["--cluster_out="], "--cluster_out needs a file name!"),
    (["--cluster_out", "s", "--cluster_table="], "--cluster_table needs a file name!"),
    (["--cluster_out", "s", "--cluster_what", "1"], "unknown option --cluster_what!"),
    (["--cluster_out", "s", "--cluster_signed=1"], "unknown option --cluster_signed!"),
    (["--cluster_out", "s", "--cluster_min_maf"], "--cluster_min_maf needs a value!"),
    (["--cluster_table"], "--cluster_table needs a value!"),
    (["--cluster_out"], "--cluster_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--cluster_out", "s", "--cluster_min_maf=-0.1"], "--cluster_min_maf must be a number >= 0!"),
    (["--cluster_out", "s", "-cluster_min_maf", "-0.1"], "--cluster_min_maf must be a number >= 0!"),
    (["--cluster_min_maf", "0.1", "--", "--cluster_out", "s"], "the --cluster_* options need --cluster_out FILE or --cluster_table FILE!"),
    (["--cluster_out", "s", "--cluster_zzz"], "unknown option --cluster_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_cluster_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not any(os.path.exists(inputs / f) for f in ("s", "t", "t.tsv"))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--cluster_out", "s"],
    ["--cluster_table", "t"],
    ["-cluster_out", "s", "--cluster_table=t", "--cluster_field", "5", "--cluster_max_kb_dist=inf", "--cluster_min_maf", "0.05",
     "--cluster_min_weight", "-0.2", "--cluster_min_size", "1", "--cluster_signed"],
    ["--cluster_out=s", "--cluster_field", "6", "--out", "t.tsv", "--prune_out", "k", "--decay_out", "b", "--site_out", "q"],
])
def test_valid_cluster_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
def test_prefixes_of_the_reference_flags_are_unchanged(inputs):
    """The --cluster_* flags are exact names taken out of argv before getopt: the reference's own abbreviations still work
    beside them ("--n_thr" is --n_threads, "--n_s" --n_sites), with and without --pos."""
    r = _run(inputs, "--cluster_out", "s", "--n_thr", "2", "--verbose", "1")
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
    argv = [capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_s", "10", "--max_kb_dist", "0", "--cluster_table", "t"]
    r = subprocess.run(argv, capture_output=True, text=True, cwd=str(inputs), timeout=120)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr, r.stderr[-500:]
