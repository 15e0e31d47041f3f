"""The binary's --cross_* flags and the ABI of ngsld_cross_ld, no GPU: every bad value is refused in the ERROR block of the
binary's other argument errors (exit -1) before any device is touched, a valid command line gets past the argument checks, the
four symbols are exported and the two versioned structs are laid out as include/ngsld.h declares them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ngsld_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    capi.build()
    d = tmp_path_factory.mktemp("cross_args")
    np.random.default_rng(1).random(10 * 4 * 3).astype("<f8").tofile(str(d / "g.bin"))
    (d / "p.pos").write_text("".join(f"{1 + i // 5}\t{(i % 5) * 10 + 1}\n" for i in range(10)))
    return d


def _run(d, *extra, pos=True):
    argv = [capi.CLI_PATH, "--geno", str(d / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--max_kb_dist", "0",
            *(["--pos", str(d / "p.pos")] if pos else []), *extra]
    return subprocess.run(argv, capture_output=True, text=True, cwd=str(d), timeout=120)


X = ["--cross_out", "s"]
LD_MSG = "--cross_ld must be a comma-separated list of r2_ExpG, D, Dp and r2!"
NEED_OUT = "the --cross_* options need --cross_out FILE!"
BIN_MSG = "--cross_bin_size must be an integer in [1, 2147483647]!"
ONE_DEVICE = "--cross_out runs on one device: it cannot be combined with --devices!"
BAD = [
    ([*X, "--cross_ld", "r3"], LD_MSG),
    ([*X, "--cross_ld", "r2,"], LD_MSG),
    ([*X, "--cross_ld", ""], LD_MSG),
    ([*X, "--cross_min_maf", "-0.1"], "--cross_min_maf must be a number >= 0!"),
    ([*X, "--cross_min_maf", "inf"], "--cross_min_maf must be a number >= 0!"),
    ([*X, "--cross_min_maf", ""], "--cross_min_maf must be a number >= 0!"),
    ([*X, "--cross_linked_min", "nan"], "--cross_linked_min must be a number!"),
    ([*X, "--cross_linked_min", "half"], "--cross_linked_min must be a number!"),
    ([*X, "--cross_linked_min="], "--cross_linked_min must be a number!"),
    ([*X, "--cross_min_kb_dist", "-1"], "--cross_min_kb_dist must be a number >= 0!"),
    ([*X, "--cross_min_kb_dist", "inf"], "--cross_min_kb_dist must be a number >= 0!"),
    ([*X, "--cross_min_kb_dist", "1kb"], "--cross_min_kb_dist must be a number >= 0!"),
    ([*X, "--devices", "0-1"], ONE_DEVICE),
    ([*X, "--cross_only", "--devices", "0,0"], ONE_DEVICE),
    (["--cross_ld", "r2"], NEED_OUT),
    (["--cross_signed"], NEED_OUT),
    (["--cross_only"], NEED_OUT),
    (["--cross_bin_size", "100"], NEED_OUT),
    (["--cross_linked_min", "0.2", "--out", "t.tsv"], NEED_OUT),
    (["--cross_out="], "--cross_out needs a file name!"),
    ([*X, "--cross_bin_size", "0"], BIN_MSG),
    ([*X, "--cross_bin_size", "2147483648"], BIN_MSG),
    ([*X, "--cross_bin_size", "1e3"], BIN_MSG),
    ([*X, "--cross_bin_size", "-5"], BIN_MSG),
    ([*X, "--cross_bin_size", "100.5"], BIN_MSG),
    ([*X, "--cross_bin_size="], BIN_MSG),
    ([*X, "--cross_what", "1"], "unknown option --cross_what!"),
    ([*X, "--cross_signed=1"], "unknown option --cross_signed!"),
    ([*X, "--cross_only=1"], "unknown option --cross_only!"),
    ([*X, "--cross_min_maf"], "--cross_min_maf needs a value!"),
    (["--cross_bin_size", "100", "--cross_out"], "--cross_out needs a value!"),
    # the forms a flag can take on the command line: --name=value, one dash, after "--" (left to getopt: not taken)
    ([*X, "--cross_min_maf=-0.1"], "--cross_min_maf must be a number >= 0!"),
    ([*X, "-cross_min_maf", "-0.1"], "--cross_min_maf must be a number >= 0!"),
    (["--cross_only", "--", "--cross_out", "s"], NEED_OUT),
]


@pytest.mark.parametrize("extra,msg", BAD, ids=[f"bad{i}" for i in range(len(BAD))])
def test_bad_cross_values_are_refused(inputs, extra, msg):
    r = _run(inputs, *extra)
    assert r.returncode == 255, (r.returncode, r.stderr[-500:])
    assert "ERROR: [" in r.stderr and msg in r.stderr, r.stderr[-500:]
    assert "ngsld_create" not in r.stderr          # refused before any device is touched
    assert not os.path.exists(inputs / "s") and not os.path.exists(inputs / "t.tsv")


def test_cross_out_without_pos_is_refused(inputs):
    r = _run(inputs, *X, pos=False)
    assert r.returncode == 255 and "ERROR: [check_cross_args] --cross_out needs positions: it cannot run without --pos!" in r.stderr
    assert "ngsld_create" not in r.stderr and not os.path.exists(inputs / "s")


@pytest.mark.parametrize("extra", [
    X,
    ["-cross_out", "s", "--cross_bin_size=2147483647", "--cross_ld", "r2_ExpG,D,Dp,r2", "--cross_min_maf", "0.05",
     "--cross_linked_min", "-0.2", "--cross_signed", "--cross_only", "--cross_min_kb_dist=2.5"],
    ["--cross_out=s", "--cross_bin_size", "1", "--cross_ld", "Dp", "--out", "t.tsv", "--prune_out", "k", "--decay_out", "b", "--grid_out", "u",
     "--grid_bin_size", "10"],
    [*X, "--n_thr", "2", "--verbose", "1"],  # (exact names taken out of argv before getopt: the reference's abbreviations still work)
])
def test_valid_cross_command_line_passes_the_argument_checks(inputs, extra, tmp_path):
    """With a GPU the run goes through; without one it gets as far as the device and says so: never an argument error."""
    r = subprocess.run([capi.CLI_PATH, "--geno", str(inputs / "g.bin"), "--n_ind", "4", "--n_sites", "10", "--max_kb_dist", "0",
                        "--pos", str(inputs / "p.pos"), *extra], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    for name in ("check_cross_args", "take_flags", "parse_cmd_args"):
        assert f"ERROR: [{name}]" not in r.stderr, r.stderr[-500:]
    if r.returncode != 0:
        assert r.returncode == 255 and "ERROR: [ngsld_create]" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(tmp_path / "s")
    else:
        assert open(tmp_path / "s").readline().startswith("chr1\tbin1\tchr2\tbin2\tn\t")


# ---- the ABI ----
CTYPE = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}


def _declared(struct):
    """[(field, ctypes type)] of a typedef struct of include/ngsld.h, in order."""
    text = open(os.path.join(REPO, "include", "ngsld.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            out += [(n.strip(), CTYPE[ctype]) for n in names.split(",")]
    return out


@pytest.mark.parametrize("struct,binding", [("ngsld_cross_ld_params", "CrossLdParams"), ("ngsld_cross_ld_stats", "CrossLdStats")])
def test_the_structs_are_the_headers(struct, binding):
    cls = getattr(capi, binding)
    assert list(cls._fields_) == _declared(struct)
    assert cls._fields_[0][0] == "struct_size" and C.sizeof(cls) % 8 == 0
    assert C.sizeof(cls) == sum(C.sizeof(t) for _, t in cls._fields_)  # (no padding: the C compiler lays it out the same way)
    if struct.endswith("stats"):
        assert {"pairs", "pairs_counted", "pairs_cross", "cells", "bins", "chunks", "span_items", "lds", "pairs_ms", "cross_ms",
                "total_ms"} <= {n for n, _ in cls._fields_}


def test_the_symbols_are_exported_and_refuse_a_null_context():
    capi.build()
    L = capi.lib()
    names = ["ngsld_cross_ld", "ngsld_cross_ld_cells", "ngsld_cross_ld_chromosomes", "ngsld_cross_ld_get"]
    assert all(n in capi.SYMBOLS and hasattr(L, n) for n in names)
    p = capi.CrossLdParams(C.sizeof(capi.CrossLdParams), 8, 0, 0.0, 0.5, 0.0, 1, 1)
    assert L.ngsld_cross_ld(None, C.byref(p), None, None) == capi.ERR_INVALID
    assert L.ngsld_cross_ld_cells(None, 0, None, None, None, None, None, None) == capi.ERR_INVALID
    assert L.ngsld_cross_ld_chromosomes(None, 0, None, None) == capi.ERR_INVALID
    assert L.ngsld_cross_ld_get(None, 7, 0, None, None, None, None) == capi.ERR_INVALID
