"""The binary's --prune_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid pruning command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("prune_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    (d / "subset.txt").write_text("1:1\n1:11\n")
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


BAD = [
    (["--prune_out", "k", "--prune_field", "3"], "--prune_field must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!"),
    (["--prune_out", "k", "--prune_field", "8"], "--prune_field must be"),
    (["--prune_out", "k", "--prune_field", "7x"], "--prune_field must be"),
    (["--prune_out", "k", "--prune_weight_type", "x"], "--prune_weight_type must be a, e or n!"),
    (["--prune_out", "k", "--prune_weight_type", "ae"], "--prune_weight_type must be a, e or n!"),
    (["--prune_out", "k", "--prune_precision", "-1"], "--prune_precision must be an integer in [0,15]!"),
    (["--prune_out", "k", "--prune_precision", "16"], "--prune_precision must be an integer in [0,15]!"),
    (["--prune_out", "k", "--prune_precision", "2.5"], "--prune_precision must be an integer in [0,15]!"),
    (["--prune_out", "k", "--prune_max_kb_dist", "-1"], "--prune_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--prune_out", "k", "--prune_max_kb_dist", "ten"], "--prune_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--prune_out", "k", "--prune_max_kb_dist", "nan"], "--prune_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--prune_out", "k", "--prune_min_weight", "0.2x"], "--prune_min_weight must be a number!"),
    (["--prune_out", "k", "--prune_min_weight", ""], "--prune_min_weight must be a number!"),
    (["--prune_out", "k", "--prune_subset", "no_such_file"], "cannot open --prune_subset file!"),
    (["--prune_out", "k", "--prune_excl="], "--prune_excl needs a file name!"),
    (["--prune_out", "k", "--devices", "0-1"], "--prune_out runs on one device: it cannot be combined with --devices!"),
    (["--prune_excl", "x"], "the --prune_* options need --prune_out FILE!"),
    (["--prune_keep_heavy"], "the --prune_* options need --prune_out FILE!"),
    (["--prune_out="], "the --prune_* options need --prune_out FILE!"),
    (["--prune_out", "k", "--prune_what", "1"], "unknown option --prune_what!"),
    (["--prune_out", "k", "--prune_field"], "--prune_field needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--prune_out", "k", "--prune_max_kb_dist=-1"], "--prune_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--prune_out", "k", "-prune_max_kb_dist", "-1"], "--prune_max_kb_dist must be a number >= 0 (or inf)!"),
    (["--prune_min_weight", "0.1", "--", "--prune_out", "k"], "the --prune_* options need --prune_out FILE!"),
    (["--prune_out", "k", "--prune_zzz"], "unknown option --prune_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_prune_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert f"ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "k")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--prune_out", "k"],
    ["-prune_out", "k", "--prune_excl", "x.gz", "--prune_field", "5", "--prune_weight_type", "e", "--prune_min_weight=-1",
     "--prune_max_kb_dist", "2.5", "--prune_keep_heavy", "--prune_precision", "6", "--prune_subset", "subset.txt"],
    ["--prune_out=k", "--prune_max_kb_dist", "inf", "--out", "t.tsv"],
])
def test_valid_prune_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]


def test_prefixes_of_the_reference_flags_are_unchanged(inputs):
    """The --prune_* flags are exact names taken out of argv before getopt: "--pr" is still --probs, "--p" still ambiguous
    among the reference's own three."""
    r = _run(inputs, "--pr", "--verbose", "1")
    assert "probs: true" in r.stderr
    r = _run(inputs, "--p", "x")
    assert "is ambiguous" in r.stderr and "prune" not in r.stderr
