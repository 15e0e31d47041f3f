"""GPU: the run kernel's Pearson cross moment and first-step dosage sum from pair_ld_moments_kernel (ld_pair_moments.hip: the
band of X X^T on the f64 matrix pipe, in front of every launch of the run kernel) against the oracle, and against the same
kernel with the pass switched off (NGSLD_TEST_PAIR_MOMENTS=0: both sums formed per pair inside the kernel, as before the pass
existed).

What can go wrong there and is held here at the smallest shapes that reach it (300 sites, 44,850 pairs, unless said): padding
individuals and the K chunks (np = 512, 192, 320, 576), sites whose alleles the kernel relabels, sites that may not take part
beside sites that do (a non-finite dosage must stay in its own row and column of the product), items with dropped candidates
(the map from tile element to record), row ends inside tiles, and the rule the suite holds bit for bit: a pair's two sums do not
depend on the tile, launch cut, batch or grid that computed them.  Bars: tests/util.py -- nIter and sample_size exact, values
to 1e-9, degenerate pairs bit for bit.
Where 1e-9 cannot see, the pass's two sums are held by tests/test_gpu_pearson_exact.py (bits) and tests/test_gpu_pearson_margin.py."""
import contextlib
import os

import numpy as np
import pytest

from ngsld_amd import capi, shard, synth
from oracle import orc
from util import TOL, check_records, close, same_bits

pytestmark = pytest.mark.gpu

VALUES = (("hap", "ext"), ("D", "std"), ("Dp", "std"), ("r2", "std"), ("r2_ExpG", "std"))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(eng, load, pd, on, kernel="run", **plan):
    """The knob is read at every launch."""
    load(eng)
    assert eng.pair_kernel() == kernel
    eng.set_pos_dist(pd)
    n = eng.plan(extend_out=True, **plan)
    with _env(NGSLD_TEST_PAIR_MOMENTS="1" if on else "0"):
        s1, s2, std, ext = eng.run()
    assert len(s1) == n
    return s1, s2, std, ext


def _field(got, name, where):
    return (got[3] if where == "ext" else got[2])[name]


def _differ(a, b):
    """Pairs on which two runs' haplotype frequencies or r2_ExpG are not the same bits."""
    return ~np.all(same_bits(a[3]["hap"], b[3]["hap"]), axis=1) | ~same_bits(a[2]["r2_ExpG"], b[2]["r2_ExpG"])


def _same_everywhere(a, b, rows=slice(None)):
    for name, where in VALUES + (("n_iter", "ext"), ("n_ind_data", "ext")):
        assert np.all(same_bits(_field(a, name, where)[rows], _field(b, name, where)[rows])), name


def _on_off(eng, load, want, pd=None, kernel="run", **plan):
    """The pass on, held to the oracle; the pass off: the same nIter on every pair, values within TOL -- and the pass must
    have been taken: it moves last bits somewhere."""
    on = _run(eng, load, pd, True, kernel, **plan)
    off = _run(eng, load, pd, False, kernel, **plan)
    for got in (on, off):
        assert np.array_equal(got[0], want["s1"]) and np.array_equal(got[1], want["s2"])
        check_records(got[2], got[3], want)
    assert np.array_equal(on[3]["n_iter"], off[3]["n_iter"])
    for name, where in VALUES:
        a, b = _field(on, name, where), _field(off, name, where)
        ok = close(a, b, TOL)
        with np.errstate(invalid="ignore"):
            print(f"{name}: largest |on - off| = {np.nanmax(np.abs(a - b)):.3e}")
        assert np.all(ok), f"{name}: {np.count_nonzero(~ok)} values differ by more than {TOL}"
    return on, off


@pytest.mark.parametrize("n_ind", [500, 192, 257, 576])
def test_padding_and_slot_counts(engine, n_ind):
    """500: eight slots, 12 padding individuals; 192: three full slots, no padding; 257: one individual in the last of five
    slots; 576: nine slots, where the kernel has no first step from dosages and the pass computes the moment alone."""
    raw = synth.make_gl_numpy(300, n_ind, 2100 + n_ind, depth=6.0)
    want = orc.Oracle(raw, n_threads=16).run()
    assert len(want) == 300 * 299 // 2
    on, off = _on_off(engine, lambda e: e.set_geno_raw(raw), want)
    assert _differ(on, off).any(), "the moments pass was not taken on any pair"


def test_relabelled_sites(engine):
    """Every other site's alleles trade places: its frequency lies in (0.5, 0.95) and the kernels relabel it -- e and d are
    formed under each site's own label on both sides of the product."""
    raw = synth.make_gl_numpy(300, 500, 2201, depth=6.0)
    raw[1::2] = raw[1::2, :, ::-1].copy()
    o = orc.Oracle(raw, n_threads=16)
    want = o.run()
    hi = o.maf > 0.5
    assert np.all((o.maf[1::2] > 0.5) & (o.maf[1::2] < 0.95)) and 100 < hi.sum() < 200
    assert set(zip(hi[want["s1"]].tolist(), hi[want["s2"]].tolist())) == {(False, False), (False, True), (True, False), (True, True)}
    on, off = _on_off(engine, lambda e: e.set_geno_raw(raw), want)
    assert _differ(on, off).any(), "the moments pass was not taken on any pair"


@pytest.mark.parametrize("skip_marks", [False, True])
def test_sites_that_take_no_part(skip_marks):
    """Three monomorphic sites, two with triples that sum to 0.9, one with an individual whose likelihoods are all 0 (its
    dosage is 0 / 0): handed over normalised.  All pairs meet the oracle.  The pairs of those six sites are the same bits in
    every field with the pass on and off: they take no first step from dosages either way, nothing of a site's non-finite
    dosages reaches them, and the kernel keeps its own order for their cross moment (r2_ExpG).  On the untouched pairs the pass
    moves last bits.  skip_marks: the launch is the kernel's SKIP variant."""
    raw = synth.make_gl_numpy(300, 192, 2301, depth=8.0)
    mono, odd, zero = [7, 150, 151], [20, 290], 40
    raw[mono] = (1.0, 0.0, 0.0)
    o = orc.Oracle(raw, n_threads=16)
    assert np.all(o.maf[mono] == 0.0)
    for s in odd:
        o.gl[s, 3::17] *= 0.9
        o.expg[s] = o.gl[s, :, 1] + 2 * o.gl[s, :, 2]
    o.gl[zero, 5] = 0.0
    o.expg[zero, 5] = 0.0
    want = o.run()
    touched = np.isin(want["s1"], mono + odd + [zero]) | np.isin(want["s2"], mono + odd + [zero])
    assert np.all(np.isnan(want["hap"][(want["s1"] == zero) | (want["s2"] == zero)]))
    with _env(NGSLD_REPLAY_SKIP=None if skip_marks else "0"):
        eng = capi.Engine(0)
    try:
        on, off = _on_off(eng, lambda e: e.set_geno_lkl(o.gl, o.maf), want)
    finally:
        eng.close()
    _same_everywhere(on, off, touched)
    assert _differ(on, off)[~touched].any(), "the moments pass was not taken on any pair"


@pytest.mark.parametrize("plan", [dict(min_maf=0.2813), dict(rnd_sample=0.3, seed=11)], ids=["min_maf", "rnd_sample"])
def test_sparse_items(engine, plan):
    """Candidates the filters dropped: the pass maps a tile's element to its record through the items' masks.  (The
    generator's frequencies lie in 0.25 .. 0.34: a third of the sites is below 0.2813.)"""
    raw = synth.make_gl_numpy(300, 500, 2401, depth=6.0)
    o = orc.Oracle(raw, n_threads=16, **plan)
    want = o.run()
    if "min_maf" in plan:
        assert 80 < np.count_nonzero(o.maf < plan["min_maf"]) < 130
    assert 5000 < len(want) < 30000
    on, off = _on_off(engine, lambda e: e.set_geno_raw(raw), want, **plan)
    assert _differ(on, off).any(), "the moments pass was not taken on any pair"


def test_banded_against_the_oracle(engine):
    """700 sites x 500 individuals, 10 kb window, gaps <= 200: some 100 candidates a row (62,392 pairs), six row blocks, every
    row block's last tiles beyond the band and every row's end inside a tile."""
    n_sites = 700
    raw = synth.make_gl_numpy(n_sites, 500, 2551, depth=6.0)
    chrs, pos = synth.make_positions(n_sites, 2551, max_gap=200)
    pd = shard.pos_dist_from_positions(chrs, pos)
    want = orc.Oracle(raw, pos_dist=pd, max_kb_dist=10, n_threads=16).run()
    per_row = np.bincount(want["s1"], minlength=n_sites)
    assert 60_000 < len(want) < 65_000 and 64 < per_row[:500].min() and per_row.max() < 128
    on, off = _on_off(engine, lambda e: e.set_geno_raw(raw), want, pd, max_kb_dist=10)
    assert _differ(on, off).any(), "the moments pass was not taken on any pair"


def test_banded_at_size(engine):
    """2,000 sites x 500 individuals, 100 kb window (the headline's shape, a million pairs): row ends fall inside tiles, most
    tiles of a row block lie beyond the band.  Pass on against pass off."""
    n_sites = 2000
    raw = synth.make_gl_numpy(n_sites, 500, 2501, depth=10.0)
    chrs, pos = synth.make_positions(n_sites, 2501, max_gap=200)
    pd = shard.pos_dist_from_positions(chrs, pos)
    on = _run(engine, lambda e: e.set_geno_raw(raw), pd, True, max_kb_dist=100)
    off = _run(engine, lambda e: e.set_geno_raw(raw), pd, False, max_kb_dist=100)
    assert len(on[0]) > 1_000_000
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[3]["n_iter"], off[3]["n_iter"]) and np.array_equal(on[3]["n_ind_data"], off[3]["n_ind_data"])
    for name, where in VALUES:
        a, b = _field(on, name, where), _field(off, name, where)
        ok = close(a, b, TOL)
        with np.errstate(invalid="ignore"):
            print(f"{name}: largest |on - off| = {np.nanmax(np.abs(a - b)):.3e}")
        assert np.all(ok), f"{name}: {np.count_nonzero(~ok)} values differ by more than {TOL}"
    assert _differ(on, off).any(), "the moments pass was not taken on any pair"


def test_position_independence():
    """A pair's records are the same bits whichever tile, grid, launch cut or batch computed its sums: one launch over all
    rows against single rows, grids of 7 workgroups, launches cut at 3,000 pairs, and batches of 700 pairs."""
    import torch
    n_sites = 300
    raw = synth.make_gl_numpy(n_sites, 500, 2601, depth=6.0)
    dev = torch.device("cuda", 0)

    def device_records(eng, r0, r1, n):
        d_std = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_ext = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        eng.run_device(r0, r1, d_std.data_ptr(), d_ext.data_ptr(), None)
        torch.cuda.synchronize()
        return d_std.cpu().numpy().view(capi.REC_STD), d_ext.cpu().numpy().view(capi.REC_EXT)

    def same(a, b, what):
        for k in (0, 1):
            for name in a[k].dtype.names:
                assert np.all(same_bits(a[k][name], b[k][name])), (what, name)

    eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(None)
        n = eng.plan(extend_out=True)
        assert n == n_sites * (n_sites - 1) // 2
        whole = device_records(eng, 0, n_sites, n)
        row_off = np.concatenate(([0], np.cumsum(np.arange(n_sites - 1, -1, -1))))
        for r in (0, 1, 127, 128, 200, 298):
            cnt = int(row_off[r + 1] - row_off[r])
            one = device_records(eng, r, r + 1, cnt)
            same((whole[0][row_off[r]:row_off[r + 1]], whole[1][row_off[r]:row_off[r + 1]]), one, f"row {r}")
        with _env(NGSLD_TEST_MAX_BLOCKS="7"):
            same(whole, device_records(eng, 0, n_sites, n), "grids of 7 workgroups")
        with _env(NGSLD_TEST_MOMENTS_PAIRS="3000"):
            same(whole, device_records(eng, 0, n_sites, n), "launches cut at 3,000 pairs")
    finally:
        eng.close()
    with _env(NGSLD_TEST_BATCH_PAIRS="700"):
        eng = capi.Engine(0)
    try:
        eng.set_geno_raw(raw)
        eng.set_pos_dist(None)
        assert eng.plan(extend_out=True) == n
        _, _, std, ext = eng.run()
    finally:
        eng.close()
    same(whole, (std, ext), "batches of 700 pairs")


def test_ignore_miss_data_is_untouched(engine):
    """--ignore_miss_data at 500 individuals is the masked kernel: no pass in front of it, the knob switches nothing."""
    raw = synth.make_gl_numpy(300, 500, 2701, depth=1.0)
    runs = []
    for on in (True, False):
        engine.set_geno_raw(raw, ignore_miss_data=True)
        assert engine.pair_kernel() == "run"
        engine.set_pos_dist(None)
        engine.plan(extend_out=True, ignore_miss_data=True)
        with _env(NGSLD_TEST_PAIR_MOMENTS="1" if on else "0"):
            runs.append(engine.run())
    assert len(runs[0][0]) == 300 * 299 // 2
    _same_everywhere(runs[0], runs[1])
