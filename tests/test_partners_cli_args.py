"""The binary's --partners_* flags, no GPU: every bad value and combination is refused in the ERROR block of the binary's other
argument errors (exit -1) before any device is touched, and a valid command line gets past the argument checks."""
import os
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("partners_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"1\t{i * 10 + 1}\n" for i in range(10)))
    (d / "q.txt").write_text("1:11\n1:51\n")
    return d


def _run(d, *extra, pos=True):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", *(["--pos", str(d / "p.pos")] if pos else []),
            *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


P = ["--partners_out", "s", "--partners_k", "3"]
NEED_OUT = "the --partners_* options need --partners_out FILE!"
NEED_K = "--partners_out needs the partners kept per site: --partners_k INT!"
K_MSG = "--partners_k must be an integer in [1,64]!"
FIELD_MSG = "--partners_field must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!"
DIST_MSG = "--partners_max_kb_dist must be a number >= 0 (or inf)!"
MAF_MSG = "--partners_min_maf must be a number >= 0!"
WEIGHT_MSG = "--partners_min_weight must be a number!"
ONE_DEVICE = "--partners_out runs on one device: it cannot be combined with --devices!"
BAD = [
    (["--partners_k", "3"], NEED_OUT),
    (["--partners_signed"], NEED_OUT),
    (["--partners_min_weight", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--partners_out=", "--partners_k", "3"], "--partners_out needs a file name!"),
    (["--partners_out", "s"], NEED_K),
    (["--partners_out", "s", "--partners_k", "0"], K_MSG),
    (["--partners_out", "s", "--partners_k", "65"], K_MSG),
    (["--partners_out", "s", "--partners_k", "-1"], K_MSG),
    (["--partners_out", "s", "--partners_k", "5.0"], K_MSG),
    (["--partners_out", "s", "--partners_k", "ten"], K_MSG),
    (["--partners_out", "s", "--partners_k="], K_MSG),
    ([*P, "--partners_field", "3"], FIELD_MSG),
    ([*P, "--partners_field", "8"], FIELD_MSG),
    ([*P, "--partners_field", "r2"], FIELD_MSG),
    ([*P, "--partners_min_weight", "nan"], WEIGHT_MSG),
    ([*P, "--partners_min_weight", "half"], WEIGHT_MSG),
    ([*P, "--partners_max_kb_dist", "-1"], DIST_MSG),
    ([*P, "--partners_max_kb_dist", "nan"], DIST_MSG),
    ([*P, "--partners_min_maf", "-0.1"], MAF_MSG),
    ([*P, "--partners_min_maf", "inf"], MAF_MSG),
    ([*P, "--partners_min_maf", "nan"], MAF_MSG),
    ([*P, "--partners_sites", "no_such_file.txt"], "cannot open --partners_sites file!"),
    ([*P, "--devices", "0-1"], ONE_DEVICE),
    ([*P, "--partners_signed", "--devices", "0,0"], ONE_DEVICE),
    ([*P, "--partners_what", "1"], "unknown option --partners_what!"),
    ([*P, "--partners_signed=1"], "unknown option --partners_signed!"),
    ([*P, "--partners_min_maf"], "--partners_min_maf needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    ([*P, "--partners_min_maf=-0.1"], MAF_MSG),
    ([*P, "-partners_min_maf", "-0.1"], MAF_MSG),
    (["--partners_k", "3", "--", "--partners_out", "s"], NEED_OUT),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_partners_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not any(os.path.exists(inputs / f) for f in ("s", "t.tsv"))


@pytest.mark.parametrize("pos", [True, False])
@pytest.mark.parametrize("extra", [
    P,
    ["-partners_out", "s", "--partners_k=64", "--partners_field=5", "--partners_min_weight", "-inf", "--partners_signed",
     "--partners_max_kb_dist=inf", "--partners_min_maf", "0.05"],
    [*P, "--partners_sites", "q.txt", "--out", "t.tsv", "--site_out", "u", "--linked_out", "l"],
    [*P, "--n_thr", "2", "--verbose", "1"],  # (exact names taken out of argv before getopt: the reference's abbreviations still work)
])
def test_valid_partners_command_line_passes_the_argument_checks(inputs, extra, pos, tmp_path):
    """With a GPU the run goes through; without one it gets as far as the device and says so: never an argument error.  The
    partners need no positions: without --pos every dist is inf and, with no limit, no row is dropped for it."""
    if "q.txt" in extra:
        extra = [str(inputs / "q.txt") if x == "q.txt" else x for x in extra]
        if not pos:
            (tmp_path / "q1.txt").write_text("2\n6\n")  # (without --pos a site is named by its 1-based index)
            extra = [str(tmp_path / "q1.txt") if x.endswith("q.txt") else x for x in extra]
    r = subprocess.run([capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_sites", "10",
                        *(["--pos", str(inputs / "p.pos")] if pos else ["--max_kb_dist", "0"]), *extra], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=120)
    for name in ("check_partners_args", "take_flags", "parse_cmd_args"):
        assert f"ERROR: [{name}]" not in r.stderr, r.stderr[-500:]
    if r.returncode != 0:
        assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(tmp_path / "s")
    else:
        assert os.path.exists(tmp_path / "s")
