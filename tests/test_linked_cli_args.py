"""The binary's --linked_* flags, no GPU: every bad value and combination is refused in the ERROR block of the binary's other
argument errors (exit -1) before any device is touched, and a valid linked-pairs command line gets past the argument checks."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("linked_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra, pos=True):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", *(["--pos", str(d / "p.pos")] if pos else []),
            *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


L = ["--linked_out", "s"]
NEED_OUT = "the --linked_* options need --linked_out FILE or --linked_outH FILE!"
FIELD_MSG = "--linked_field must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!"
DIST_MSG = "--linked_max_kb_dist must be a number >= 0 (or inf)!"
MAF_MSG = "--linked_min_maf must be a number >= 0!"
WEIGHT_MSG = "--linked_min_weight must be a number!"
ONE_DEVICE = "--linked_out runs on one device: it cannot be combined with --devices!"
BAD = [
    ([*L, "--linked_field", "3"], FIELD_MSG),
    ([*L, "--linked_field", "8"], FIELD_MSG),
    ([*L, "--linked_field", "r2"], FIELD_MSG),
    ([*L, "--linked_field", ""], FIELD_MSG),
    ([*L, "--linked_field", "7.0"], FIELD_MSG),
    ([*L, "--linked_min_weight", "nan"], WEIGHT_MSG),
    ([*L, "--linked_min_weight", "half"], WEIGHT_MSG),
    ([*L, "--linked_min_weight="], WEIGHT_MSG),
    ([*L, "--linked_max_kb_dist", "-1"], DIST_MSG),
    ([*L, "--linked_max_kb_dist", "nan"], DIST_MSG),
    ([*L, "--linked_max_kb_dist", "10kb"], DIST_MSG),
    ([*L, "--linked_min_maf", "-0.1"], MAF_MSG),
    ([*L, "--linked_min_maf", "inf"], MAF_MSG),
    ([*L, "--linked_min_maf", "nan"], MAF_MSG),
    ([*L, "--linked_min_maf", ""], MAF_MSG),
    ([*L, "--devices", "0-1"], ONE_DEVICE),
    (["--linked_outH", "s", "--linked_signed", "--devices", "0,0"], ONE_DEVICE),
    (["--linked_field", "7"], NEED_OUT),
    (["--linked_signed"], NEED_OUT),
    (["--linked_min_weight", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--linked_out", "s", "--linked_outH", "s2"], "--linked_out and --linked_outH cannot be combined!"),
    (["--linked_outH=s", "--linked_out=s2", "--linked_field", "5"], "--linked_out and --linked_outH cannot be combined!"),
    (["--linked_out="], "--linked_out needs a file name!"),
    (["--linked_outH="], "--linked_outH needs a file name!"),
    ([*L, "--linked_what", "1"], "unknown option --linked_what!"),
    ([*L, "--linked_signed=1"], "unknown option --linked_signed!"),
    ([*L, "--linked_min_maf"], "--linked_min_maf needs a value!"),
    (["--linked_field", "7", "--linked_out"], "--linked_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    ([*L, "--linked_min_maf=-0.1"], MAF_MSG),
    ([*L, "-linked_min_maf", "-0.1"], MAF_MSG),
    (["--linked_field", "7", "--", "--linked_out", "s"], NEED_OUT),
    ([*L, "--linked_zzz"], "unknown option --linked_zzz!"),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_linked_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not any(os.path.exists(inputs / f) for f in ("s", "s2", "t.tsv"))


@pytest.mark.parametrize("pos", [True, False])
@pytest.mark.parametrize("extra", [
    L,
    ["--linked_outH", "s"],
    ["-linked_out", "s", "--linked_field=5", "--linked_min_weight", "-inf", "--linked_signed", "--linked_max_kb_dist=inf", "--linked_min_maf",
     "0.05"],
    ["--linked_out=s.gz", "--linked_min_weight", "0", "--out", "t.tsv", "--prune_out", "k", "--decay_out", "b", "--site_out", "u", "--cluster_out",
     "v"],
    [*L, "--n_thr", "2", "--verbose", "1"],  # (exact names taken out of argv before getopt: the reference's abbreviations still work)
])
def test_valid_linked_command_line_passes_the_argument_checks(inputs, extra, pos, tmp_path):
    """With a GPU the run goes through; without one it gets as far as the device and says so: never an argument error.  The
    linked pairs need no positions: without --pos (and so without a window) every dist is inf and, with no limit, no row is
    dropped for it."""
    if not pos and "--cluster_out" in extra:
        extra = extra[:extra.index("--prune_out")]  # (the other analyses have their own needs)
    r = subprocess.run([capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_sites", "10",
                        *(["--pos", str(inputs / "p.pos")] if pos else ["--max_kb_dist", "0"]), *extra], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    for name in ("check_linked_args", "take_flags", "parse_cmd_args"):
        assert f"ERROR: [{name}]" not in r.stderr, r.stderr[-500:]
    if r.returncode != 0:
        assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(tmp_path / "s") and not os.path.exists(tmp_path / "s.gz")
    else:
        assert os.path.exists(tmp_path / "s") or os.path.exists(tmp_path / "s.gz")
