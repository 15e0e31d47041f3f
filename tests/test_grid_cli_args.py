"""The binary's --grid_* flags, no GPU: every bad value is refused in the ERROR block of the binary's other argument errors
(exit -1) before any device is touched, and a valid grid command line gets past the argument checks."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("grid_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra, pos=True):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", *(["--pos", str(d / "p.pos")] if pos else []),
            *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


G = ["--grid_out", "s", "--grid_bin_size", "100"]
LD_MSG = "--grid_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
NEED_OUT = "the --grid_* options need --grid_out FILE!"
NEED_BIN = "--grid_out needs the window in bp: --grid_bin_size INT!"
BIN_MSG = "--grid_bin_size must be an integer in [1, 2147483647]!"
ONE_DEVICE = "--grid_out runs on one device: it cannot be combined with --devices!"
BAD = [
    ([*G, "--grid_ld", "r3"], LD_MSG),
    ([*G, "--grid_ld", "r2,"], LD_MSG),
    ([*G, "--grid_ld", ""], LD_MSG),
    ([*G, "--grid_ld", "r2 Dp"], LD_MSG),
    ([*G, "--grid_max_kb_dist", "-1"], "--grid_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*G, "--grid_max_kb_dist", "nan"], "--grid_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*G, "--grid_max_kb_dist", "10kb"], "--grid_max_kb_dist must be a number >= 0 (or inf)!"),
    ([*G, "--grid_min_maf", "-0.1"], "--grid_min_maf must be a number >= 0!"),
    ([*G, "--grid_min_maf", "inf"], "--grid_min_maf must be a number >= 0!"),
    ([*G, "--grid_min_maf", ""], "--grid_min_maf must be a number >= 0!"),
    ([*G, "--grid_linked_min", "nan"], "--grid_linked_min must be a number!"),
    ([*G, "--grid_linked_min", "half"], "--grid_linked_min must be a number!"),
    ([*G, "--grid_linked_min="], "--grid_linked_min must be a number!"),
    ([*G, "--devices", "0-1"], ONE_DEVICE),
    ([*G, "--grid_signed", "--devices", "0,0"], ONE_DEVICE),
    (["--grid_ld", "r2"], NEED_OUT),
    (["--grid_signed"], NEED_OUT),
    (["--grid_bin_size", "100"], NEED_OUT),
    (["--grid_linked_min", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--grid_out=", "--grid_bin_size", "100"], "--grid_out needs a file name!"),
    (["--grid_out", "s"], NEED_BIN),
    (["--grid_out", "s", "--grid_ld", "Dp"], NEED_BIN),
    (["--grid_out", "s", "--grid_bin_size", "0"], BIN_MSG),
    (["--grid_out", "s", "--grid_bin_size", "2147483648"], BIN_MSG),
    (["--grid_out", "s", "--grid_bin_size", "1e3"], BIN_MSG),
    (["--grid_out", "s", "--grid_bin_size", "-5"], BIN_MSG),
    (["--grid_out", "s", "--grid_bin_size", "100.5"], BIN_MSG),
    (["--grid_out", "s", "--grid_bin_size="], BIN_MSG),
    ([*G, "--grid_what", "1"], "unknown option --grid_what!"),
    ([*G, "--grid_signed=1"], "unknown option --grid_signed!"),
    ([*G, "--grid_min_maf"], "--grid_min_maf needs a value!"),
    (["--grid_bin_size", "100", "--grid_out"], "--grid_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    ([*G, "--grid_min_maf=-0.1"], "--grid_min_maf must be a number >= 0!"),
    ([*G, "-grid_min_maf", "-0.1"], "--grid_min_maf must be a number >= 0!"),
    (["--grid_bin_size", "100", "--", "--grid_out", "s"], "the --grid_* options need --grid_out FILE!"),
    ([*G, "--grid_zzz"], "unknown option --grid_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_grid_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t.tsv")


def test_grid_out_without_pos_is_refused(inputs):
    r = _run(inputs, *G, "--max_kb_dist", "0", pos=False)
    assert r.returncode == 255 and "ERROR: [check_grid_args] --grid_out needs positions: it cannot run without --pos!" in r.stderr
    assert "ngsld_create" not in r.stderr and not os.path.exists(inputs / "s")


@pytest.mark.parametrize("extra", [
    G,
    ["-grid_out", "s", "--grid_bin_size=2147483647", "--grid_ld", "r2_ExpG,D,Dp,r2", "--grid_max_kb_dist=inf", "--grid_min_maf", "0.05",
     "--grid_linked_min", "-0.2", "--grid_signed"],
    ["--grid_out=s", "--grid_bin_size", "1", "--grid_ld", "Dp", "--out", "t.tsv", "--prune_out", "k", "--decay_out", "b", "--site_out", "u",
     "--cluster_out", "v"],
    [*G, "--n_thr", "2", "--verbose", "1"],  # (exact names taken out of argv before getopt: the reference's abbreviations still work)
])
def test_valid_grid_command_line_passes_the_argument_checks(inputs, extra, tmp_path):
    """With a GPU the run goes through; without one it gets as far as the device and says so: never an argument error."""
    r = subprocess.run([capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--pos", str(inputs / "p.pos"),
                        *extra], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    for name in ("check_grid_args", "take_flags", "parse_cmd_args"):
        assert f"ERROR: [{name}]" not in r.stderr, r.stderr[-500:]
    if r.returncode != 0:
        assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(tmp_path / "s")
    else:
        assert open(tmp_path / "s").readline().startswith("chr\tbin1\tbin2\tn\t")
