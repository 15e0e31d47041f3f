"""ngsld_decay and ngsld_decay_map against what the tree computed before the two calls came to share one bin kernel, one bin
plan and one column-to-means routine: tests/golden/decay_family/parent.json holds, per case and call, the integer stats, the
SHA-256 of every getter array's raw bytes, the first three bins as hex floats, and the code and text of the refusals the two
calls share and of their two size caps.  The tree must reproduce every entry exactly.  Also: on one chromosome ngsld_decay and
ngsld_decay_map(window 0) are the same kernel reached through two hosts, and return the same bytes.

The input is the suite's small one: 300 sites x 16 individuals in two chromosomes, no window, all 44,850 pairs.

    python tests/test_gpu_decay_family_golden.py record [PATH]     writes the fixture (run once, on a GPU, at the parent commit)
"""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from ngsld_amd import capi, shard, synth  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(REPO, "tests", "golden", "decay_family", "parent.json")
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
N_SITES, N_IND, W = 300, 16, 4000  # a chromosome of 150 sites spans some 22 kb: several windows of 4 kb
KNOBS = ("DECAY_LDS_BYTES", "DECAY_CHUNK_PAIRS", "DMAP_LDS_BYTES", "DMAP_CHUNK_PAIRS", "RECORD_SLICE_ITEMS", "SUM_WRAP_LIMIT")
CHRS, POS = synth.make_positions(N_SITES, 37, max_gap=300, n_chr=2)
LABELS = [f"{c}:{int(p)}" for c, p in zip(CHRS, POS)]
ONE_CHR, ONE_POS = synth.make_positions(N_SITES, 37, max_gap=300, n_chr=1)
# a dist of the table that max_kb_dist states exactly: the filter is strict, the rows at it are out
LIMIT = next(int(POS[k] - POS[0]) for k in range(60, 150) if (float(POS[k] - POS[0]) / 1000) * 1000 == float(POS[k] - POS[0]))

INPUTS = {  # name: (synth kw, chromosomes, positions)
    "two_chr": ({}, CHRS, POS),
    "mono": (dict(mono_frac=0.2), CHRS, POS),  # un-called: rows with a NaN or an inf drop out
    "one_chr": ({}, ONE_CHR, ONE_POS),
}
# name: (input, keywords of both calls, knobs).  A knob's value: "exact" / "exact-1" = (1 + fields) * bin_slots * 8 bytes (less
# one), "tenth" = pairs // 10; the LDS and chunk knobs go to both calls under their own names.
CASES = {
    "r2_lds": ("two_chr", {}, {}),
    "all4_lds": ("two_chr", dict(ld=ALL4), {}),
    "r2_bin2_global": ("two_chr", dict(bin_size=2), {}),
    "all4_bin2_global": ("two_chr", dict(ld=ALL4, bin_size=2), {}),
    "all4_maf_limit": ("two_chr", dict(ld=ALL4, min_maf=0.05, max_kb_dist=LIMIT / 1000), {}),
    "r2_maf_limit": ("two_chr", dict(min_maf=0.05, max_kb_dist=LIMIT / 1000), {}),
    "all4_lds_exact": ("two_chr", dict(ld=ALL4), dict(LDS_BYTES="exact")),
    "all4_lds_one_less": ("two_chr", dict(ld=ALL4), dict(LDS_BYTES="exact-1")),
    "all4_lds_chunks_slices": ("two_chr", dict(ld=ALL4), dict(CHUNK_PAIRS="tenth", RECORD_SLICE_ITEMS="7")),
    "all4_bin2_chunks_slices": ("two_chr", dict(ld=ALL4, bin_size=2), dict(CHUNK_PAIRS="tenth", RECORD_SLICE_ITEMS="7")),
    "all4_tracking": ("two_chr", dict(ld=ALL4), dict(SUM_WRAP_LIMIT=str(2 ** 63))),
    "all4_bin2_tracking": ("two_chr", dict(ld=ALL4, bin_size=2), dict(SUM_WRAP_LIMIT=str(2 ** 63))),
    "all4_chunk_below_a_row": ("two_chr", dict(ld=ALL4), dict(CHUNK_PAIRS="100")),  # rows of up to 299 pairs: decay's per-chunk track_max
    "r2_mono": ("mono", {}, {}),
    "all4_mono": ("mono", dict(ld=ALL4), {}),
    "all4_mono_bin2_chunks": ("mono", dict(ld=ALL4, bin_size=2), dict(CHUNK_PAIRS="tenth", RECORD_SLICE_ITEMS="7")),
}
_made = {}


def _raw(name):
    return synth.make_gl_numpy(N_SITES, N_IND, 500 + N_SITES + N_IND, depth=4.0, **INPUTS[name][0])


def _new_engine(name, pos_dist=None, plan=True):
    eng = capi.Engine(0)
    eng.set_geno_raw(_raw(name))
    eng.set_pos_dist(shard.pos_dist_from_positions(INPUTS[name][1], INPUTS[name][2]) if pos_dist is None else pos_dist)
    if plan:
        assert eng.plan(extend_out=True) == N_SITES * (N_SITES - 1) // 2
    return eng


def _engine(name):
    if name not in _made:
        _made[name] = _new_engine(name)
    return _made[name]


def _close_all():
    for eng in _made.values():
        eng.close()
    _made.clear()


def _set_knobs(knobs, fields, probe):
    for k in KNOBS:
        os.environ.pop("NGSLD_TEST_" + k, None)
    exact = (1 + fields) * probe["bin_slots"] * 8
    value = {"exact": str(exact), "exact-1": str(exact - 1), "tenth": str(probe["pairs"] // 10)}
    for k, v in knobs.items():
        for name in (("DECAY_" + k, "DMAP_" + k) if k in ("LDS_BYTES", "CHUNK_PAIRS") else (k,)):
            os.environ["NGSLD_TEST_" + name] = value.get(v, v)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _first_bins(dist, count, mean):
    return [[float(dist[k]).hex(), int(count[k])] + [float(x).hex() for x in mean[k]] for k in range(min(3, len(dist)))]


def _decay_entry(bins, st):
    names = [f for f in ALL4 if f in bins]
    mean = np.stack([bins[f] for f in names], axis=1)  # [bin][field], as ngsld_decay_bins hands it out
    return {"stats": {k: int(st[k]) for k in ("pairs", "pairs_counted", "bins", "bin_slots", "lds")},
            "sha256": {"dist": _sha(bins["dist"]), "count": _sha(bins["n"]), "mean": _sha(mean)},
            "first_bins": _first_bins(bins["dist"], bins["n"], mean)}


def _map_entry(eng, st, fields):
    """The raw arrays of the three getters of ngsld_decay_map."""
    L, h = eng._L, eng._h
    n_chr, ng, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    eng._check(L.ngsld_decay_map_chromosomes(h, 0, None, C.byref(n_chr)))
    names = (C.c_char_p * max(int(n_chr.value), 1))()
    eng._check(L.ngsld_decay_map_chromosomes(h, int(n_chr.value), names, None))
    eng._check(L.ngsld_decay_map_groups(h, 0, None, None, None, None, C.byref(ng)))
    eng._check(L.ngsld_decay_map_bins(h, 0, None, None, None, C.byref(nb)))
    ng, nb = int(ng.value), int(nb.value)
    chr_ = np.zeros(ng, dtype=np.uint32)
    win, first, length = (np.zeros(ng, dtype=np.uint64) for _ in range(3))
    dist, count, mean = np.zeros(nb), np.zeros(nb, dtype=np.uint64), np.zeros((nb, fields))
    eng._check(L.ngsld_decay_map_groups(h, ng, chr_.ctypes.data, win.ctypes.data, first.ctypes.data, length.ctypes.data, None))
    eng._check(L.ngsld_decay_map_bins(h, nb, dist.ctypes.data, count.ctypes.data, mean.ctypes.data, None))
    return {"stats": {k: int(st[k]) for k in ("pairs", "pairs_counted", "bins", "bin_slots", "lds", "groups")},
            "chromosomes": [names[k].decode() for k in range(int(n_chr.value))],
            "sha256": {"chr": _sha(chr_), "win_start": _sha(win), "first_bin": _sha(first), "n_bins": _sha(length),
                       "dist": _sha(dist), "count": _sha(count), "mean": _sha(mean)},
            "first_bins": _first_bins(dist, count, mean)}


def _case(name):
    inp, kw, knobs = CASES[name]
    eng = _engine(inp)
    fields = len(kw.get("ld", ("r2",)))
    try:
        _set_knobs({}, fields, dict(bin_slots=0, pairs=0))
        _, probe = eng.decay(**kw)
        _set_knobs(knobs, fields, probe)
        out = {"decay": _decay_entry(*eng.decay(**kw))}
        for tag, window in (("map_chromosome", 0), ("map_window", W)):
            _, st = eng.decay_map(LABELS, window=window, **kw)
            out[tag] = _map_entry(eng, st, fields)
    finally:
        _set_knobs({}, fields, dict(bin_slots=0, pairs=0))
    assert out["decay"]["stats"]["pairs_counted"] > 0 and out["map_window"]["stats"]["groups"] > out["map_chromosome"]["stats"]["groups"] == 2
    return out


def _analyze_case():
    """Decay as one kind of ngsld_analyze, next to site LD."""
    res, _ = _engine("two_chr").analyze(decay=dict(ld=ALL4), site_ld=dict(ld=("r2",)))
    return {"decay": _decay_entry(*res["decay"])}


# ---- refusals: (code, text) of both calls ----
def _refusal(eng, call, labels=None, struct_size=None, fields=8, bin_size=250.0, max_kb_dist=math.inf, min_maf=0.0, window=0):
    if call == "decay":
        p = capi.DecayParams(C.sizeof(capi.DecayParams) if struct_size is None else struct_size, fields, bin_size, max_kb_dist, min_maf)
        st = capi.DecayStats()
        st.struct_size = C.sizeof(capi.DecayStats)
        rc = eng._L.ngsld_decay(eng._h, C.byref(p), C.byref(st))
    else:
        p = capi.DecayMapParams(C.sizeof(capi.DecayMapParams) if struct_size is None else struct_size, fields, bin_size, max_kb_dist,
                                min_maf, window)
        st = capi.DecayMapStats()
        st.struct_size = C.sizeof(capi.DecayMapStats)
        arr = None if labels is None else (C.c_char_p * len(labels))(*[l.encode() for l in labels])
        rc = eng._L.ngsld_decay_map(eng._h, C.byref(p), arr, C.byref(st))
    assert rc != capi.OK
    return [rc, eng._L.ngsld_last_error(eng._h).decode()]


SHARED_REFUSALS = {
    "fields_0": dict(fields=0), "fields_16": dict(fields=16), "bin_size_1": dict(bin_size=1.0), "bin_size_inf": dict(bin_size=math.inf),
    "bin_size_nan": dict(bin_size=math.nan), "max_kb_dist_negative": dict(max_kb_dist=-1.0), "max_kb_dist_nan": dict(max_kb_dist=math.nan),
    "min_maf_nan": dict(min_maf=math.nan), "struct_size": dict(struct_size=8),
}


def _refusals():
    out = {}
    eng = _engine("two_chr")
    for name, kw in SHARED_REFUSALS.items():
        out[name] = {call: _refusal(eng, call, **kw) for call in ("decay", "decay_map")}
    eng = _new_engine("two_chr", plan=False)
    try:
        out["not_planned"] = {call: _refusal(eng, call) for call in ("decay", "decay_map")}
    finally:
        eng.close()
    eng = _new_engine("two_chr", pos_dist=np.full(N_SITES, 10.5))  # half a base between sites: a finite limit is refused
    try:
        out["limit_needs_integer_gaps"] = {call: _refusal(eng, call, max_kb_dist=0.5) for call in ("decay", "decay_map")}
    finally:
        eng.close()
    # the two size caps.  ngsld_decay: a bin size just above 1 on chromosomes of 150 sites 40 kb apart (6 * 10^6 bp > 2^22);
    # refused in prepare, before any kernel runs.  ngsld_decay_map: windows of 1 bp over positions up to 10^9.
    spread = np.concatenate([np.arange(1, 151) * 40_000] * 2)
    eng = _new_engine("two_chr", pos_dist=shard.pos_dist_from_positions(CHRS, spread))
    try:
        out["decay_bin_cap"] = {"decay": _refusal(eng, "decay", bin_size=1.000001)}
    finally:
        eng.close()
    labels = [f"{c}:{(k + 1) * 4_500_000}" for k, c in enumerate(CHRS)]
    out["decay_map_accumulator_cap"] = {"decay_map": _refusal(_engine("two_chr"), "decay_map", labels=labels, window=1, bin_size=2.0)}
    return out


def _record(path):
    try:
        doc = {"cases": {name: _case(name) for name in CASES}, "analyze": _analyze_case(), "refusals": _refusals()}
    finally:
        _close_all()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(f"{path}: {len(doc['cases'])} cases, {len(doc['refusals'])} refusals")


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    _close_all()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_fixture_covers_every_case(parent):
    assert set(parent["cases"]) == set(CASES) and set(parent["refusals"]) >= set(SHARED_REFUSALS) | {
        "not_planned", "limit_needs_integer_gaps", "decay_bin_cap", "decay_map_accumulator_cap"}
    lds = {name: c["decay"]["stats"]["lds"] for name, c in parent["cases"].items()}
    assert lds["all4_lds_exact"] == 1 and lds["all4_lds_one_less"] == 0 and lds["r2_bin2_global"] == 0 and lds["r2_lds"] == 1
    assert all(c["decay"]["stats"]["lds"] == c["map_window"]["stats"]["lds"] for c in parent["cases"].values())
    assert "more than 2^22 decay bins" in parent["refusals"]["decay_bin_cap"]["decay"][1]
    assert "pass 1 GiB of accumulators" in parent["refusals"]["decay_map_accumulator_cap"]["decay_map"][1]


@pytest.mark.parametrize("name", list(CASES))
def test_case_reproduces_the_parent(parent, name):
    got = _case(name)
    for call, want in parent["cases"][name].items():
        assert got[call] == want, (name, call)


def test_decay_in_analyze_reproduces_the_parent(parent):
    assert _analyze_case() == parent["analyze"]
    assert parent["analyze"]["decay"] == parent["cases"]["all4_lds"]["decay"]  # (the single call's answer)


def test_refusals_reproduce_the_parent(parent):
    got = _refusals()
    assert got == parent["refusals"]
    eng = _engine("two_chr")  # the context is usable after them
    assert _decay_entry(*eng.decay()) == parent["cases"]["r2_lds"]["decay"]


@pytest.mark.parametrize("form", ["lds", "global"])
def test_one_chromosome_is_the_same_bytes_from_both_calls(form):
    """One kernel behind two hosts: decay's one-group site table against the map's per-chromosome table, under small chunks
    and slices (launches of fewer items than workgroups, spans that do not divide evenly)."""
    eng = _engine("one_chr")
    kw = dict(ld=ALL4, bin_size=250 if form == "lds" else 2)
    labels = [f"{c}:{int(p)}" for c, p in zip(ONE_CHR, ONE_POS)]
    try:
        _set_knobs({}, 4, dict(bin_slots=0, pairs=0))
        _, probe = eng.decay(**kw)
        _set_knobs(dict(CHUNK_PAIRS="tenth", RECORD_SLICE_ITEMS="7"), 4, probe)
        bins, st = eng.decay(**kw)
        groups, mst = eng.decay_map(labels, window=0, **kw)
    finally:
        _set_knobs({}, 4, dict(bin_slots=0, pairs=0))
    assert st["lds"] == mst["lds"] == (1 if form == "lds" else 0) and st["chunks"] > 5 and mst["chunks"] > 5
    assert len(groups) == 1 and st["pairs_counted"] == mst["pairs_counted"] > 0
    assert set(bins) | {"chr", "win_start"} == set(groups[0])
    for k in bins:
        assert bins[k].tobytes() == groups[0][k].tobytes(), k


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "record":
        sys.exit(__doc__)
    _record(sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
