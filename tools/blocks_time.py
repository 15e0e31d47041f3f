"""LD blocks on one MI355X: the phases of ngsld_blocks on BASELINE configs[2] at full size (100,000 sites x 500 individuals,
100 kb window) and on its un-called twin (20 % monomorphic sites), for regions of about 1,000, 5,000 and 20,000 sites, with
r2,Dp and with all four statistics; the bytes and the time of each matrix file; and the binary's wall time with --blocks_out
alone against --out.

    python tools/blocks_time.py [OUT_DIR]       (default profiles/blocks; one JSON document, also printed)
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from ngsld_amd import capi, shard, synth  # noqa: E402

ALL4 = ("r2_ExpG", "D", "Dp", "r2")
N_SITES, N_IND, MAX_KB = 100_000, 500, 100
REGIONS = (1_000, 5_000, 20_000)
FIRST = 40_000


def text_bytes(eng, field):
    """ngsld_blocks_text into a counting sink: (bytes, format_ms, host_rows, wall_s)."""
    n = [0]

    def sink(_user, _text, k):
        n[0] += k
        return 0

    st = capi.BlocksStats()
    st.struct_size = C.sizeof(capi.BlocksStats)
    t0 = time.perf_counter()
    eng._check(eng._L.ngsld_blocks_text(eng._h, 4 + ALL4.index(field), capi.TEXT_FN(sink), None, C.byref(st)))
    return n[0], st.format_ms, st.host_rows, time.perf_counter() - t0


def timed_blocks(raw, chrs, pos):
    eng = capi.Engine(0)
    out = {}
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(shard.pos_dist_from_positions(chrs, pos))
        out["pairs"] = eng.plan(max_kb_dist=MAX_KB, extend_out=False)
        t0 = time.perf_counter()
        eng.run_discard()                                   # the pair phase of every row once (warm-up, and for scale)
        out["run_discard_all_rows_s"] = time.perf_counter() - t0
        labels = [f"{c}:{int(p)}" for c, p in zip(chrs, pos)]
        for k in REGIONS:
            start, end = int(pos[FIRST]), int(pos[FIRST + k - 1])
            for name, ld in (("r2_Dp", ("r2", "Dp")), ("all4", ALL4)):
                st = None
                for _ in range(2):                          # (the second call is the one reported: warm caches and allocator)
                    t0 = time.perf_counter()
                    _, _, st = _blocks_only(eng, labels, start, end, ld)
                    st["wall_s"] = time.perf_counter() - t0
                st["region"] = [start, end]
                st["text"] = {}
                for f in ld:
                    b, fmt_ms, host_rows, wall = text_bytes(eng, f)
                    st["text"][f] = {"bytes": b, "format_ms": fmt_ms, "host_rows": host_rows, "wall_s": wall,
                                     "GB_per_s": b / 1e9 / max(fmt_ms / 1e3, 1e-9)}
                out[f"sites_{k}_{name}"] = st
    finally:
        eng.close()
    return out


def _blocks_only(eng, labels, start, end, ld):
    """ngsld_blocks without copying the matrices out (Engine.blocks copies every matrix to the host)."""
    mask = sum(1 << ALL4.index(f) for f in ld)
    arr = (C.c_char_p * len(labels))(*[l.encode() for l in labels])
    p = capi.BlocksParams(C.sizeof(capi.BlocksParams), mask, b"chr1", start, end)
    st = capi.BlocksStats()
    st.struct_size = C.sizeof(capi.BlocksStats)
    eng._check(eng._L.ngsld_blocks(eng._h, C.byref(p), arr, C.byref(st)))
    return None, None, {k: getattr(st, k) for k, _ in capi.BlocksStats._fields_ if k not in ("struct_size", "reserved")}


def binary_wall(raw, chrs, pos, d):
    g, p = os.path.join(d, "g.bin"), os.path.join(d, "p.pos")
    raw.astype("<f8").tofile(g)
    synth.write_pos(p, chrs, pos)
    base = [capi.CLI_PATH, "--geno", g, "--n_ind", str(N_IND), "--n_sites", str(len(chrs)), "--pos", p, "--max_kb_dist",
            str(MAX_KB)]
    res = {}
    t0 = time.perf_counter()
    r = subprocess.run(base + ["--out", "/dev/null"], capture_output=True, text=True, timeout=600)
    res["out_tsv_s"] = time.perf_counter() - t0
    if r.returncode != 0:
        res["out_tsv_error"] = r.stderr[-1000:]
    for k in REGIONS:
        start, end = int(pos[FIRST]), int(pos[FIRST + k - 1])
        prefix = os.path.join(d, "B")
        t0 = time.perf_counter()
        r = subprocess.run(base + ["--blocks_out", prefix, "--blocks_chr", "chr1", "--blocks_start", str(start), "--blocks_end",
                                   str(end)], capture_output=True, text=True, timeout=600)
        res[f"blocks_out_{k}_s"] = time.perf_counter() - t0
        if r.returncode != 0:
            res[f"blocks_out_{k}_error"] = r.stderr[-1000:]
        else:
            res[f"blocks_out_{k}_stderr"] = [ln for ln in r.stderr.splitlines() if "LD blocks" in ln]
            res[f"blocks_out_{k}_bytes"] = sum(os.path.getsize(f"{prefix}.{f}.tsv") for f in ("r2", "Dp"))
        for f in ("r2", "Dp"):
            if os.path.exists(f"{prefix}.{f}.tsv"):
                os.unlink(f"{prefix}.{f}.tsv")
    return res


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "blocks")
    os.makedirs(out_dir, exist_ok=True)
    res = {}
    chrs, pos = synth.make_positions(N_SITES, 2, max_gap=200)
    raw = synth.make_gl_numpy(N_SITES, N_IND, 2, depth=10.0)
    res["configs2"] = timed_blocks(raw, chrs, pos)
    with tempfile.TemporaryDirectory() as d:
        res["configs2_binary"] = binary_wall(raw, chrs, pos, d)
    del raw
    twin = synth.make_gl_numpy(N_SITES, N_IND, 2, depth=10.0, mono_frac=0.2)
    res["configs2_uncalled_twin"] = timed_blocks(twin, chrs, pos)
    del twin
    txt = json.dumps(res, indent=1, default=float)
    print(txt)
    with open(os.path.join(out_dir, "blocks_time.json"), "w") as fh:
        fh.write(txt + "\n")


if __name__ == "__main__":
    main()
