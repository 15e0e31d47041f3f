"""The binary's --tree_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid tree command line gets as far as the device."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("tree_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(d / "p.pos"), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


FIELD_MSG = "--tree_field must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!"
NEED_OUT = "the --tree_* options need --tree_out FILE or --tree_cut_out FILE!"
KB_MSG = "--tree_max_kb_dist must be a number >= 0 (or inf)!"
MAF_MSG = "--tree_min_maf must be a number >= 0!"
W_MSG = "--tree_min_weight must be a number!"
CUT_MSG = "--tree_cut must be a comma-separated list of numbers!"
LOW_MSG = "--tree_cut cannot go below --tree_min_weight: the tree holds no edge under it!"
DEV_MSG = "--tree_out runs on one device: it cannot be combined with --devices!"
BAD = [
    (["--tree_out", "s", "--tree_field", "3"], FIELD_MSG),
    (["--tree_out", "s", "--tree_field", "8"], FIELD_MSG),
    (["--tree_out", "s", "--tree_field", "r2"], FIELD_MSG),
    (["--tree_out", "s", "--tree_field", ""], FIELD_MSG),
    (["--tree_out", "s", "--tree_field", "7.0"], FIELD_MSG),
    (["--tree_out", "s", "--tree_min_weight", "nan"], W_MSG),
    (["--tree_out", "s", "--tree_min_weight", "half"], W_MSG),
    (["--tree_out", "s", "--tree_min_weight="], W_MSG),
    (["--tree_out", "s", "--tree_max_kb_dist", "-1"], KB_MSG),
    (["--tree_out", "s", "--tree_max_kb_dist", "nan"], KB_MSG),
    (["--tree_out", "s", "--tree_max_kb_dist", "10kb"], KB_MSG),
    (["--tree_out", "s", "--tree_min_maf", "-0.1"], MAF_MSG),
    (["--tree_out", "s", "--tree_min_maf", "inf"], MAF_MSG),
    (["--tree_out", "s", "--tree_min_maf", ""], MAF_MSG),
    (["--tree_cut_out", "t", "--tree_cut", ""], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5,"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", ",0.5"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5,,0.2"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5;0.2"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5,nan"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5, 0.2x"], CUT_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5,0.09"], LOW_MSG),                                   # (the default floor is 0.1)
    (["--tree_cut_out", "t", "--tree_cut", "0.3", "--tree_min_weight", "0.300001"], LOW_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "-0.3", "--tree_signed"], LOW_MSG),
    (["--tree_out", "s", "--tree_cut", "0.5"], "--tree_cut needs --tree_cut_out FILE!"),
    (["--tree_out", "s", "--tree_cut_out", "t"], "--tree_cut_out needs the floors to cut at: --tree_cut T1,T2,...!"),
    (["--tree_out", "s", "--devices", "0-1"], DEV_MSG),
    (["--tree_cut_out", "t", "--tree_cut", "0.5", "--tree_signed", "--devices", "0,0"], DEV_MSG),
    (["--tree_field", "7"], NEED_OUT),
    (["--tree_signed"], NEED_OUT),
    (["--tree_cut", "0.5"], NEED_OUT),
    (["--tree_min_weight", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--tree_min_maf", "0.1", "--cluster_out", "s"], NEED_OUT),
    (["--tree_out="], "--tree_out needs a file name!"),
    (["--tree_out", "s", "--tree_cut", "0.5", "--tree_cut_out="], "--tree_cut_out needs a file name!"),
    (["--tree_out", "s", "--tree_what", "1"], "unknown option --tree_what!"),
    (["--tree_out", "s", "--tree_signed=1"], "unknown option --tree_signed!"),
    (["--tree_out", "s", "--tree_min_maf"], "--tree_min_maf needs a value!"),
    (["--tree_cut_out"], "--tree_cut_out needs a value!"),
    (["--tree_out"], "--tree_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    (["--tree_out", "s", "--tree_min_maf=-0.1"], MAF_MSG),
    (["--tree_out", "s", "-tree_min_maf", "-0.1"], MAF_MSG),
    (["--tree_min_maf", "0.1", "--", "--tree_out", "s"], NEED_OUT),
    (["--tree_out", "s", "--tree_zzz"], "unknown option --tree_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_tree_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not any(os.path.exists(inputs / f) for f in ("s", "t", "t.tsv"))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU exit")
@pytest.mark.parametrize("extra", [
    ["--tree_out", "s"],
    ["--tree_cut_out", "t", "--tree_cut", "0.8,0.5,0.2"],
    ["-tree_out", "s", "--tree_cut_out=t", "--tree_cut=1e-1,.5,inf", "--tree_field", "5", "--tree_max_kb_dist=inf", "--tree_min_maf", "0.05",
     "--tree_min_weight", "-0.2", "--tree_signed"],
    ["--tree_out=s", "--tree_field", "6", "--out", "t.tsv", "--prune_out", "k", "--cluster_out", "b", "--site_out", "q"],
])
def test_valid_tree_command_line_reaches_the_device(inputs, extra):
    r = _run(inputs, *extra)
    assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t")


def test_the_binding_knows_the_tree():
    L = capi.lib()
    names = ("ngsld_ld_tree", "ngsld_ld_tree_merges", "ngsld_ld_tree_cut")
    assert all(n in capi.SYMBOLS and hasattr(L, n) for n in names)
