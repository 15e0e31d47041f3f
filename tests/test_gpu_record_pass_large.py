"""The large-job paths of the six record passes -- LD pruning, decay, blocks, site LD, clusters and the grid -- at small shapes.

The passes' own files and tests/test_gpu_analyses_by_family.py hold them to their plain-Python rules on jobs of some 50,000 pairs.
Four things of their host frame (RecordPass, record_pass.h) and of their kernels turn on only from 2^24 or 2^25 pairs or items,
which is where the headline job (100,000 x 500, 9.9e7 pairs) runs; three test knobs (knobs.h) bring them down to 500 sites:

* NGSLD_TEST_PRUNE_CHUNK_PAIRS: ngsld_prune in many chunks -- the edge arrays regrown between chunks, the edge count carried on
  the host, out_base moving -- and its refusal of a row that does not fit the record buffer;
* NGSLD_TEST_RECORD_SLICE_ITEMS: a chunk's items in many launches, a slice beginning inside a row and inside a 16-row tile of
  the LDS forms of site_kernel and grid_kernel, which clip every tile to the launch's items;
* NGSLD_TEST_SUM_WRAP_LIMIT = L: the guard of the integer sums.  Site LD, grid, clusters and decay track max |q| in every lane,
  fold it into meta[1] and the host refuses a sum from max |q| * rows >= L on (2^63 as shipped).  With M the largest |q| the
  rule counts and N the bound of rows the host uses -- both restated here, M from the table and N from the plan --, L = M * N must
  be refused and L = M * N + 1 accepted: a max that misses one lane, one slice or one chunk lets M * N pass.  The input is chosen
  so that the one pair holding M lies outside the first chunk, outside the first slice of its chunk and not in lane 0 of its item;
* chunk knobs of 1: every row a chunk of its own, the buffer sized to the longest row (the four passes that accept such a row, and
  the blocks).

Every result is held bit for bit to the pass's rule on the same engine's TSV (prune_ref, decay_ref, site_ref, cluster_ref, grid_ref,
blocks_ref) and byte for byte to the same call with no knob set.  No tolerances.

GPU time of this file on one MI355X: see README.md (the tests row)."""
import collections
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import blocks_ref
import cluster_ref
import decay_ref
import grid_ref
import prune_ref
import site_ref
from ngsld_amd import capi, shard, synth
from test_gpu_clusters import _same as _same_clusters
from test_gpu_decay import _same as _same_decay
from test_gpu_grid import _same as _same_grid
from test_gpu_site_ld import _same as _same_site_ld

pytestmark = pytest.mark.gpu

# The seed and the guard's fields were chosen on the CPU, from the oracle's table of this input (the oracle prints the same
# values): of seeds 71 .. 74 and the four statistics, seed 71 has its largest |D'| -- 1.493066, rounding noise of an un-called
# monomorphic site -- in ONE pair, (434, 475): row 434 of 500 (the ninth of ten chunks), 40 candidates into its item.  Its largest
# r2 lies in row 20 and its largest |D| and r2_ExpG in lane 0: a max taken from the first chunk or from lane 0 alone would find them.
SEED = 71
N_SITES, N_IND = 500, 64
PLANS = {
    "window": dict(max_kb_dist=20, extend_out=True),
    "sparse": dict(max_kb_dist=20, extend_out=True, rnd_sample=0.3, seed=7),  # (items with sparse masks)
}
ALL4 = ("r2_ExpG", "D", "Dp", "r2")
GRID_BIN = 2000
TILE_ROWS = 16  # (kTileRows of site_ld.hip and grid.hip)
KW = {
    "prune": dict(min_weight=0.3, weight_type="a"),
    "decay": dict(ld=ALL4, bin_size=33.3),
    "blocks": dict(ld=ALL4),
    "site_ld": dict(ld=ALL4, abs_value=False, linked_min=0.3),
    "clusters": dict(field=7, min_weight=0.5, min_size=1),
    "grid": dict(ld=ALL4, abs_value=False, linked_min=0.3),
}
# the guard: D' is the second of two chosen fields, so the kernels' loop over the fields has to reach it
GUARD_LD = ("D", "Dp")
GUARD_KW = {
    "decay": dict(ld=GUARD_LD, bin_size=33.3),
    "site_ld": dict(ld=GUARD_LD, abs_value=True, linked_min=0.3),
    "clusters": dict(field=6, min_weight=1.0, min_size=1),  # (ten clusters; the one of the most edges is not the first with edges)
    "grid": dict(ld=GUARD_LD, abs_value=True, linked_min=0.3),
}
CHUNK_KNOB = {"prune": "PRUNE_CHUNK_PAIRS", "decay": "DECAY_CHUNK_PAIRS", "blocks": "BLOCKS_CHUNK_PAIRS", "site_ld": "SITE_CHUNK_PAIRS",
              "clusters": "CLUSTER_CHUNK_PAIRS", "grid": "GRID_CHUNK_PAIRS"}
KNOBS = tuple(CHUNK_KNOB.values()) + ("RECORD_SLICE_ITEMS", "SUM_WRAP_LIMIT", "SITE_LDS_BYTES", "GRID_LDS_BYTES", "DECAY_LDS_BYTES",
                                      "PRUNE_HOST_AFTER", "BLOCKS_HOST_ROWS", "BLOCKS_TEXT_ROWS")
REFUSAL = {"site_ld": "a site in up to {} pairs", "grid": "a grid cell of up to {} pairs", "clusters": "a cluster of {} edges",
           "decay": "a row of {} pairs"}


@contextlib.contextmanager
def _knobs(**knobs):
    """The record passes' test knobs set to `knobs` (names without NGSLD_TEST_) and to nothing else; put back after."""
    before = {k: os.environ.get("NGSLD_TEST_" + k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop("NGSLD_TEST_" + k, None)
        for k, v in knobs.items():
            assert k in KNOBS, k
            os.environ["NGSLD_TEST_" + k] = str(v)
        yield
    finally:
        for k, v in before.items():
            os.environ.pop("NGSLD_TEST_" + k, None)
            if v is not None:
                os.environ["NGSLD_TEST_" + k] = v


Row = collections.namedtuple("Row", "s1 s2 dist q maf_ok")  # dist None: not finite; q: micro-units of the four fields, None: nan / inf


class Job:
    """The input under one plan: the engine's own TSV, its rows read back, the plan's rows and work items."""

    def __init__(self, plan):
        self.plan = plan
        self.raw = synth.make_gl_numpy(N_SITES, N_IND, SEED, depth=4.0, mono_frac=0.1)
        self.chrs, self.pos = synth.make_positions(N_SITES, SEED, max_gap=300, n_chr=2)
        self.labels = [f"{c}:{int(p)}" for c, p in zip(self.chrs, self.pos)]
        self.text = None
        with _knobs(), self.engine() as eng:
            row_off, row_end = eng.plan_rows()
            self.items = eng.items()
        self.row_off, self.row_end = [int(x) for x in row_off], [int(x) for x in row_end]
        self.row_pairs = [b - a for a, b in zip(self.row_off, self.row_off[1:])]
        assert self.row_off[-1] == self.n_pairs
        # the items lie row by row: item_off[r] of them before row r
        s1 = self.items["s1"].astype(np.int64)
        assert np.all(np.diff(s1) >= 0)
        self.item_off = [int(x) for x in np.searchsorted(s1, np.arange(N_SITES + 1))]
        index = {lab: k for k, lab in enumerate(self.labels)}
        self.rows = []
        for ln in self.text.splitlines():
            if not ln or ln.startswith("site1\t"):
                continue
            f = ln.split("\t")
            dist = None if f[2].strip().lstrip("+-").lower() in ("inf", "nan") else int(f[2])
            mafs = [site_ref.micro(f[8]), site_ref.micro(f[9])]
            self.rows.append(Row(index[f[0]], index[f[1]], dist, [site_ref.micro(f[k]) for k in (3, 4, 5, 6)],
                                 all(m is not None and site_ref.printed(m) >= 0.0 for m in mafs)))
        assert len(self.rows) == self.n_pairs and [r.s1 for r in self.rows] == sorted(r.s1 for r in self.rows)
        # a region strictly inside chr1 that starts and ends mid-row-range (tests/test_gpu_analyses_by_family.py's)
        p1 = np.sort(np.array([p for c, p in zip(self.chrs, self.pos) if c == "chr1"]))
        self.region = (int(p1[len(p1) // 4]) + 1, int(p1[len(p1) * 3 // 5]))
        self.member = [c == "chr1" and self.region[0] <= p <= self.region[1] for c, p in zip(self.chrs, self.pos)]

    @contextlib.contextmanager
    def engine(self):
        eng = capi.Engine(0)
        try:
            eng.set_geno_raw(self.raw)
            eng.set_pos_dist(shard.pos_dist_from_positions(self.chrs, self.pos))
            self.n_pairs = eng.plan(**PLANS[self.plan])
            # Every engine writes the TSV first, as the binary does before its analyses and as the engines of
            # tests/test_gpu_analyses_by_family.py do.  The last bits of a record the replay settles (never its text) depend on who
            # settled it, and the device takes over from the host once a context has replayed a few thousand pairs: the block
            # matrices, which hold the records' own doubles, are compared between calls that both come after that.  The sampled
            # plan flags too few pairs a run for that: there the device is asked to replay from the first flagged pair on.
            if self.plan == "sparse":
                eng.set_exact_store(2)
            eng.set_text_output(self.labels)
            text, fallbacks = eng.run_text()
            assert fallbacks == 0
            if self.text is None:
                self.text = text.decode()
            assert text.decode() == self.text
            yield eng
        finally:
            eng.close()

    def chunks(self, chunk_pairs, rows=None):
        """RecordPass's rule, restated from plan_rows() as tests/test_gpu_grid.py does: consecutive rows (of `rows`, when given)
        while their pairs fit chunk_pairs, a row never cut; [(r0, r1, pairs)] of the chunks with pairs."""
        out, r = [], 0
        while r < N_SITES:
            if rows is not None and not rows[r]:
                r += 1
                continue
            e = r + 1
            while e < N_SITES and (rows is None or rows[e]) and self.row_off[e + 1] - self.row_off[r] <= chunk_pairs:
                e += 1
            if self.row_off[e] > self.row_off[r]:
                out.append((r, e, self.row_off[e] - self.row_off[r]))
            r = e
        return out

    def item_of(self, s1, s2):
        """(index, lane) of the work item and the lane that hold the pair."""
        for i in range(self.item_off[s1], self.item_off[s1 + 1]):
            it = self.items[i]
            lane = s2 - int(it["s2_begin"])
            if 0 <= lane < int(it["count"]) and (int(it["mask"]) >> lane) & 1:
                return i, lane
        raise AssertionError((s1, s2))


@functools.lru_cache(maxsize=None)
def _job(plan):
    return Job(plan)


# ---- the passes: run, the result as bytes, the result held to the rule ----
def _run(eng, job, name, kw):
    """(result, stats) of one pass."""
    if name == "prune":
        return eng.prune(job.labels, **{k: (list(v) if k == "subset" else v) for k, v in kw.items()})
    if name == "decay":
        return eng.decay(**kw)
    if name == "site_ld":
        return eng.site_ld(**kw)
    if name == "grid":
        return eng.grid(job.labels, GRID_BIN, **kw)
    if name == "clusters":
        ids, table, stats = eng.clusters(**kw)
        return (ids, table), stats
    assert name == "blocks"
    sites, mats, stats = eng.blocks(job.labels, "chr1", job.region[0], job.region[1], ld=kw["ld"])
    return (sites, mats, {f: eng.blocks_text(f) for f in kw["ld"]}), stats


def _arrays(d):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in d.items()}


def _bytes(name, res):
    if name == "prune":
        return {"state": res.tobytes()}
    if name == "clusters":
        return {"ids": res[0].tobytes(), **_arrays(res[1])}
    if name == "blocks":
        sites, mats, texts = res
        return {"sites": sites.tobytes(), **{f"text_{f}": t for f, t in texts.items()},
                **{f"values_{f}": m[0].tobytes() for f, m in mats.items()}, **{f"present_{f}": m[1].tobytes() for f, m in mats.items()}}
    return _arrays(res)


def _frozen(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _want(plan, name, frozen_kw):
    """The rule on the TSV, once per (plan, pass, parameters)."""
    job, kw = _job(plan), dict(frozen_kw)
    if name == "prune":
        if "subset" in kw:
            kw["subset"] = set(kw["subset"])
        return prune_ref.prune_tsv_counts(job.text, **kw)
    if name == "decay":
        return decay_ref.decay_bins(job.text, **kw)
    if name == "site_ld":
        return site_ref.site_ld(job.text, job.labels, **kw)
    if name == "grid":
        return grid_ref.grid(job.text, job.labels, GRID_BIN, **kw)
    if name == "clusters":
        return cluster_ref.clusters(job.text, job.labels, **{**kw, "min_size": 1})
    assert name == "blocks"
    return blocks_ref.blocks(job.text, "chr1", job.region[0], job.region[1], ld=kw["ld"])


def _hold(job, name, kw, res, stats):
    """The result against the rule, bit for bit, and the stats' counts against the table's."""
    want = _want(job.plan, name, _frozen(kw))
    if name != "blocks":
        assert stats["pairs"] == job.n_pairs
    if name == "prune":
        kept, excl, nodes, edges = want
        got_kept = {job.labels[k] for k in np.nonzero(res == 1)[0]}
        got_excl = {job.labels[k] for k in np.nonzero(res == 2)[0]}
        assert got_kept == kept and got_excl == excl, (len(got_kept ^ kept), len(got_excl ^ excl))
        assert stats["nodes"] == stats["kept"] + stats["excluded"] == nodes == len(kept) + len(excl)
        assert stats["edges"] == edges, (stats["edges"], edges)
    elif name == "decay":
        _same_decay(res, want, kw["ld"])
        assert stats["bins"] == len(want) > 0 and stats["pairs_counted"] == sum(w[1] for w in want) > 0
    elif name == "site_ld":
        _same_site_ld(res, want, kw["ld"])
        assert stats["pairs_counted"] * 2 == sum(want["n"]) > 0 and stats["sites_with_pairs"] == sum(1 for x in want["n"] if x)
        if job.plan == "window":
            assert stats["pairs_counted"] < stats["pairs"]  # (the NaN and inf rows of the un-called monomorphic sites drop out)
    elif name == "grid":
        _same_grid(res, want, kw["ld"])
        assert stats["pairs_counted"] == sum(want["n"]) > 0 and stats["cells"] == len(want["n"])
    elif name == "clusters":
        want_ids, want_all = want
        _same_clusters(res[0], res[1], want_ids, [r for r in want_all if r["size"] >= kw["min_size"]])
        assert stats["nodes"] == sum(1 for k in want_ids if k) and stats["edges"] == sum(r["edges"] for r in want_all) > 0
        assert stats["clusters"] == len(want_all) == max(want_ids, default=0)
    else:
        want_sites, files, info = want
        sites, mats, texts = res
        assert [job.labels[s] for s in sites] == want_sites and len(want_sites) > 20
        assert stats["sites"] == info["sites"] and stats["pairs_in_region"] == info["pairs_in_region"] > 0
        assert stats["pairs"] == sum(p for p, m in zip(job.row_pairs, job.member) if m)
        for f in kw["ld"]:
            assert texts[f].decode() == files[f], f


def _same_bytes(name, got, base):
    assert got.keys() == base.keys()
    for k in got:
        assert got[k] == base[k], (name, k)


@functools.lru_cache(maxsize=None)
def _base(plan, name, frozen_kw):
    """(bytes, stats) of a pass with no knob set, held to its rule: what every knobbed run must reproduce."""
    job, kw = _job(plan), dict(frozen_kw)
    with _knobs(), job.engine() as eng:
        res, stats = _run(eng, job, name, kw)
    _hold(job, name, kw, res, stats)
    if "chunks" in stats:
        assert stats["chunks"] == 1
    return _bytes(name, res), stats


def _knobbed(eng, job, name, kw, knobs, hold=True):
    """A pass under `knobs`: the bytes of the un-knobbed call, and held to the rule again; returns the stats."""
    with _knobs(**knobs):
        res, stats = _run(eng, job, name, kw)
    _same_bytes(name, _bytes(name, res), _base(job.plan, name, _frozen(kw))[0])
    if hold:
        _hold(job, name, kw, res, stats)
    return stats


def _refused(eng, job, name, kw, knobs, *words):
    with _knobs(**knobs), pytest.raises(capi.NgsldError) as e:
        _run(eng, job, name, kw)
    assert e.value.code == capi.ERR_UNSUPPORTED and all(w in e.value.msg for w in words), (e.value.code, e.value.msg, words)


# ---- 1. ngsld_prune in chunks ----
PRUNE_CHUNK = 1000
PRUNE_CASES = {
    # name: (plan, parameters).  A floor of 0: nearly every pair of one chromosome is an edge and the arrays regrow chunk after
    # chunk; 0.3: a few thousand edges, the first chunk's room lasts
    "floor0_abs": ("window", dict(min_weight=0.0, weight_type="a")),
    "floor0.3_abs": ("window", dict(min_weight=0.3, weight_type="a")),
    "floor0_unit_weights": ("window", dict(min_weight=0.0, weight_type="n")),
    "signed_D": ("window", dict(field=5, min_weight=-1.0, weight_type="e")),  # (negative labels: the host rule, flagged in any chunk)
    "floor0.3_keep_heavy": ("window", dict(min_weight=0.3, weight_type="a", keep_heavy=True)),
    "floor0_subset": ("window", dict(min_weight=0.0, weight_type="a", subset="every third")),
    "floor0_sparse": ("sparse", dict(min_weight=0.0, weight_type="a")),
}


@pytest.mark.parametrize("case", list(PRUNE_CASES))
def test_prune_in_chunks(case):
    plan, kw = PRUNE_CASES[case]
    job = _job(plan)
    if kw.get("subset") == "every third":
        kw = {**kw, "subset": tuple(job.labels[::3])}
    assert max(job.row_pairs) < PRUNE_CHUNK < job.n_pairs // 10
    chunks = job.chunks(PRUNE_CHUNK)
    assert len(chunks) > 10 and sum(c[2] for c in chunks) == job.n_pairs
    base, st0 = _base(plan, "prune", _frozen(kw))
    with job.engine() as eng:
        st = _knobbed(eng, job, "prune", kw, {"PRUNE_CHUNK_PAIRS": PRUNE_CHUNK})
        last = eng.last_kernel_time()[2]  # (the pairs of the last ngsld_run_device: the last chunk's)
        with _knobs():
            eng.prune(job.labels, **{k: (list(v) if k == "subset" else v) for k, v in kw.items()})
            whole = eng.last_kernel_time()[2]
    print(f"{case}: pairs {st['pairs']} nodes {st['nodes']} edges {st['edges']} excluded {st['excluded']} rounds {st['rounds']} host_nodes "
          f"{st['host_nodes']}, {len(chunks)} chunks of up to {PRUNE_CHUNK} pairs, the last of {last}")
    assert last == chunks[-1][2] < st["pairs"] and whole == st["pairs"]
    assert {k: st[k] for k in ("pairs", "nodes", "edges", "kept", "excluded")} == {k: st0[k] for k in ("pairs", "nodes", "edges", "kept", "excluded")}
    if case == "floor0_abs":
        assert st["edges"] > job.n_pairs // 2  # (more edges than any doubling of the first chunk's room holds: the arrays regrow)
    if case == "floor0.3_abs":
        assert 0 < st["edges"] < job.n_pairs // 4
    if "subset" in kw:
        assert 0 < st["nodes"] <= len(kw["subset"])


def test_prune_refuses_a_row_longer_than_its_chunk():
    job, kw = _job("window"), KW["prune"]
    longest = max(job.row_pairs)
    base, _ = _base("window", "prune", _frozen(kw))
    with job.engine() as eng:
        _refused(eng, job, "prune", kw, {"PRUNE_CHUNK_PAIRS": longest - 1}, "does not fit the record buffer", f"a row of {longest} pairs")
        with _knobs():
            state, _ = eng.prune(job.labels, **kw)  # (the refusal leaves the context usable)
        assert state.tobytes() == base["state"]
        _knobbed(eng, job, "prune", kw, {"PRUNE_CHUNK_PAIRS": longest})  # (the longest row fits exactly)


# ---- 2. a chunk's items in several launches ----
PASSES = ("prune", "decay", "blocks", "site_ld", "clusters", "grid")
LDS, GLOBAL = {"SITE_LDS_BYTES": 65536, "GRID_LDS_BYTES": 65536}, {"SITE_LDS_BYTES": 0, "GRID_LDS_BYTES": 0}
SLICE_CASES = {
    # name: (plan, items a slice, small chunks, the LDS knobs)
    "slice7_lds": ("window", 7, False, LDS),
    "slice64_lds": ("window", 64, False, LDS),
    "slice7_global": ("window", 7, False, GLOBAL),
    "slice64_global": ("window", 64, False, GLOBAL),
    "slice7_chunks_lds": ("window", 7, True, LDS),
    "slice64_chunks_lds": ("window", 64, True, LDS),
    "slice7_chunks_global": ("window", 7, True, GLOBAL),
    "sparse_slice7_lds": ("sparse", 7, False, LDS),
    "sparse_slice64_chunks_lds": ("sparse", 64, True, LDS),
}


def _slice_starts(job, chunks, slice_items):
    """The first item of every launch but a chunk's first one, with its chunk: [(item, r0, r1)]."""
    return [(i, r0, r1) for r0, r1, _ in chunks for i in range(job.item_off[r0] + slice_items, job.item_off[r1], slice_items)]


@pytest.mark.parametrize("case", list(SLICE_CASES))
def test_slices_give_the_same_bytes(case):
    plan, slice_items, small_chunks, lds = SLICE_CASES[case]
    job = _job(plan)
    chunk = job.n_pairs // 10 if small_chunks else None
    # where the launches begin: some strictly inside a row, and (so) strictly inside a tile of 16 rows counted from the chunk's first
    chunks = job.chunks(chunk or job.n_pairs)
    starts = _slice_starts(job, chunks, slice_items)
    in_row = sum(1 for i, _, _ in starts if job.item_off[int(job.items[i]["s1"])] < i)
    in_tile = sum(1 for i, r0, r1 in starts
                  if job.item_off[r0 + (int(job.items[i]["s1"]) - r0) // TILE_ROWS * TILE_ROWS] < i)
    assert len(chunks) == (1 if chunk is None else len(chunks)) and (chunk is None or len(chunks) > 5)
    assert len(starts) >= 8 and in_row > 0 and in_tile >= in_row, (len(starts), in_row, in_tile)
    assert slice_items % 4 != 0 or slice_items == 64
    if plan == "sparse":  # (items mostly empty: far more items than pairs / 64, masks with holes)
        masks = job.items["mask"]
        full = (np.uint64(1) << job.items["count"].astype(np.uint64)) - np.uint64(1)
        assert int(np.count_nonzero(masks != full)) > len(masks) // 2 and len(masks) * 64 > 2 * job.n_pairs
    with job.engine() as eng:
        for name in PASSES:
            kw = KW[name]
            knobs = {"RECORD_SLICE_ITEMS": slice_items, **lds}
            if chunk is not None:
                pairs = sum(p for p, m in zip(job.row_pairs, job.member) if m) if name == "blocks" else job.n_pairs
                knobs[CHUNK_KNOB[name]] = pairs // 10
            st = _knobbed(eng, job, name, kw, knobs)
            if "chunks" in st:
                assert (st["chunks"] > 5) if chunk is not None else (st["chunks"] == 1), (name, st["chunks"])
            if name in ("site_ld", "grid"):
                assert st["lds"] == (1 if lds is LDS else 0), name
            if name == "clusters":
                assert st["union_launches"] == sum(-(-(job.item_off[r1] - job.item_off[r0]) // slice_items) for r0, r1, _ in chunks)
    print(f"{case}: {len(chunks)} chunk(s), {len(starts) + len(chunks)} launches a pass, {in_row} begin inside a row, {in_tile} inside a tile")


# ---- 3. a row per chunk ----
def test_every_row_a_chunk_of_its_own():
    """Chunks of 1 pair: below the shortest row, so every row with pairs is a chunk and the record buffer is sized to the
    longest row (fit_longest_row).  Decay tracks max |q| in every row longer than its chunk, as it does in a row beyond 2^24."""
    job = _job("window")
    rows_with_pairs = sum(1 for p in job.row_pairs if p)
    assert min(p for p in job.row_pairs if p) >= 1 and max(job.row_pairs) > 100
    with job.engine() as eng:
        for name in ("decay", "site_ld", "clusters", "grid", "blocks"):
            st = _knobbed(eng, job, name, KW[name], {CHUNK_KNOB[name]: 1})
            want = sum(1 for p, m in zip(job.row_pairs, job.member) if p and m) if name == "blocks" else rows_with_pairs
            assert st["chunks"] == want > 50, (name, st["chunks"], want)
        st = _knobbed(eng, job, "site_ld", KW["site_ld"], {"SITE_CHUNK_PAIRS": 1, "SITE_LDS_BYTES": 0, "RECORD_SLICE_ITEMS": 1})
        assert st["chunks"] == rows_with_pairs and st["lds"] == 0


# ---- 4. the guard of the integer sums ----
def _counted(job, name, kw):
    """The rows the rule of `name` counts with their largest |q| over the chosen fields: [(row, |q|)]."""
    if name == "clusters":
        _, edges = cluster_ref.tsv_edges(job.text, job.labels, **{k: v for k, v in kw.items() if k != "min_size"})
        q_of = {(a, b): abs(q) for a, b, q in edges}
        return [(r, q_of[(r.s1, r.s2)]) for r in job.rows if (r.s1, r.s2) in q_of]
    fields = [k for k, f in enumerate(ALL4) if f in kw["ld"]]
    out = []
    for r in job.rows:
        if r.dist is None or not r.maf_ok or any(r.q[k] is None for k in fields) or (name == "decay" and not r.dist > 0):
            continue
        out.append((r, max(abs(r.q[k]) for k in fields)))
    return out


def _bound(job, name, kw):
    """N: the rows a sum of the pass can hold, as the host bounds them -- restated from the plan, the labels and the table."""
    if name == "site_ld":  # a site's own row, and the rows whose candidate range [r + 1, row_end[r]) covers it
        return max(job.row_pairs[s] + sum(1 for r in range(s) if job.row_pairs[r] and r + 1 <= s < job.row_end[r]) for s in range(N_SITES))
    if name == "grid":  # the two largest bin populations p1 >= p2: p1 * p2 between two bins, p1 * (p1 - 1) / 2 inside one
        pop = sorted(collections.Counter((c, int(p) // GRID_BIN) for c, p in zip(job.chrs, job.pos)).values())
        return min(max(pop[-1] * pop[-2], pop[-1] * (pop[-1] - 1) // 2), job.n_pairs)
    if name == "clusters":
        return max(r["edges"] for r in _want(job.plan, "clusters", _frozen(kw))[1])
    raise AssertionError(name)


def _decay_check(job, counted, chunk):
    """ngsld_decay's check after every chunk: the largest |q| of the chunks so far x this chunk's pairs.  [(pairs, product)]"""
    out, top = [], 0
    for r0, r1, pairs in job.chunks(chunk):
        top = max([top] + [q for r, q in counted if r0 <= r.s1 < r1])
        out.append((pairs, top * pairs))
    return out


GUARD_CASES = {
    # name: (small chunks, items a slice)
    "one_chunk": (False, None),
    "chunks": (True, None),
    "slices": (False, 7),
    "chunks_slices": (True, 7),
}


@pytest.mark.parametrize("case", list(GUARD_CASES))
@pytest.mark.parametrize("name", ["site_ld", "grid", "clusters", "decay"])
def test_sum_guard_is_pinned_to_the_unit(name, case):
    small_chunks, slice_items = GUARD_CASES[case]
    job, kw = _job("window"), GUARD_KW[name]
    chunk = job.n_pairs // 10 if small_chunks else None
    knobs = {"GRID_LDS_BYTES": 65536} if case != "chunks" else {"GRID_LDS_BYTES": 0, "SITE_LDS_BYTES": 0}
    if chunk is not None:
        knobs[CHUNK_KNOB[name]] = chunk
    if slice_items is not None:
        knobs["RECORD_SLICE_ITEMS"] = slice_items
    base, _ = _base("window", name, _frozen(kw))

    # M from the table, N from the plan; where the pair holding M lies
    counted = _counted(job, name, kw)
    M = max(q for _, q in counted)
    holders = [r for r, q in counted if q == M]
    want = _want("window", name, _frozen(kw))
    if name in ("site_ld", "grid"):  # (abs_value: the rule's own maxima are of |q|)
        assert M == max(x for f in kw["ld"] for x in want[f"max_{f}"] if x is not None)
    chunks = job.chunks(chunk or job.n_pairs)
    if name == "decay":
        checks = _decay_check(job, counted, chunk or job.n_pairs)
        T = max(p for _, p in checks)
        N_at = lambda L: next(pairs for pairs, p in checks if p >= L)  # noqa: E731  (the first chunk the host refuses)
        assert T >= M * min(c[2] for c in chunks)
    else:
        N = _bound(job, name, kw)
        T = M * N
        N_at = lambda L: N  # noqa: E731
    assert M > 0 and T < 2 ** 63
    if case == "chunks_slices":
        # the bracket bites: a max of the first chunk, of a chunk's first launch or of lane 0 alone does not hold M
        assert len(holders) == 1
        for r in holders:
            i, lane = job.item_of(r.s1, r.s2)
            r0 = next(a for a, b, _ in chunks if a <= r.s1 < b)
            assert r.s1 >= chunks[0][1] and i - job.item_off[r0] >= slice_items and i >= slice_items and lane != 0, (r.s1, r.s2, i, lane, r0)
            rest = [(x, q) for x, q in counted if x is not r]
            assert max(q for _, q in rest) < M
            if name == "decay":  # (without that pair no chunk's check reaches T)
                assert max(p for _, p in _decay_check(job, rest, chunk)) < T
        if name == "clusters":  # (the cluster of the most edges is not the first one the host meets)
            table = want[1]
            assert next(t["edges"] for t in table if t["edges"]) < N
    print(f"{name} {case}: M {M} in {[(r.s1, r.s2) for r in holders[:3]]}, refused from {T} on (N {N_at(T)}), {len(chunks)} chunk(s)")

    phrase = REFUSAL[name]
    with job.engine() as eng:
        st = _knobbed(eng, job, name, kw, {**knobs, "SUM_WRAP_LIMIT": 2 ** 63})  # (tracking on, the shipped limit)
        if "chunks" in st:
            assert (st["chunks"] > 5) == small_chunks
        _refused(eng, job, name, kw, {**knobs, "SUM_WRAP_LIMIT": 1}, phrase.format(N_at(1)), "too large to sum exactly")
        _refused(eng, job, name, kw, {**knobs, "SUM_WRAP_LIMIT": T}, phrase.format(N_at(T)), "too large to sum exactly")
        # a refusal leaves no result behind ...
        L = eng._L
        if name == "clusters":
            assert L.ngsld_clusters_sites(eng._h, None) == capi.ERR_INVALID
            assert L.ngsld_clusters_table(eng._h, 1, 0, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
        if name == "grid":
            assert L.ngsld_grid_cells(eng._h, 0, None, None, None, None, None) == capi.ERR_INVALID
            assert L.ngsld_grid_chromosomes(eng._h, 0, None, None) == capi.ERR_INVALID
            assert L.ngsld_grid_get(eng._h, 6, 0, None, None, None, None) == capi.ERR_INVALID
        if name == "site_ld":
            assert L.ngsld_site_ld_get(eng._h, 6, None, None, None, None, None) == capi.ERR_INVALID
        if name == "decay":
            got = C.c_uint64(7)
            assert L.ngsld_decay_bins(eng._h, 0, None, None, None, C.byref(got)) == capi.OK and got.value == 0
        # ... and the context usable: one unit more is accepted, with the un-knobbed bytes
        _knobbed(eng, job, name, kw, {**knobs, "SUM_WRAP_LIMIT": T + 1}, hold=False)
        _knobbed(eng, job, name, kw, {}, hold=False)
