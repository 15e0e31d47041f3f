"""GPU: a run that ends in an error leaves nothing queued behind it (engine_run.hip: BatchRun::run, group_text_to_sink, run_grouped).

The error is a sink that fails on its third batch -- an ordinary return code -- with many small batches, so that later batches
are in flight on the compute, text and copy streams when it fails.  The same engine then runs the same input again: its slots'
buffers are the ones the failed run's batches were writing, so the records or the text are a fresh engine's only if that run
was waited for before ngsld_run returned."""
import numpy as np
import pytest

from ngsld_amd import capi, shard, synth
from test_gpu_replay_lkl import uncalled

pytestmark = pytest.mark.gpu

N_SITES, N_IND, MAX_KB = 300, 20, 2

ROUTES = {
    "records_direct": ({}, False, False),
    "records_copied": ({"NGSLD_TEST_RUN_DIRECT": "0"}, False, False),
    "records_two_streams": ({"NGSLD_TEST_RUN_STREAMS": "2"}, False, False),
    "text_called": ({}, True, False),
    "text_uncalled_groups": ({"NGSLD_TEST_TEXT_GROUP_PAIRS": "2048"}, True, True),
}


@pytest.fixture(scope="module")
def inputs():
    chrs, pos = synth.make_positions(N_SITES, 41, max_gap=200)
    return {
        "called": synth.make_gl_numpy(N_SITES, N_IND, seed=41, depth=6.0),
        "uncalled": uncalled(N_SITES, N_IND, seed=41, depth=8.0, mono_frac=0.25),
        "pd": shard.pos_dist_from_positions(chrs, pos),
        "labels": [f"{c}:{p}" for c, p in zip(chrs, pos)],
    }


def _prepared(inputs, text, un_called):
    e = capi.Engine(0)                      # (the batch, route and stream knobs are read when the context is made)
    e.set_geno_raw(inputs["uncalled" if un_called else "called"])
    e.set_pos_dist(inputs["pd"])
    n = e.plan(max_kb_dist=MAX_KB, extend_out=True)
    assert 3000 < n < 20000
    if text:
        e.set_text_output(inputs["labels"])
    return e


def _ordinary(e, text):
    if text:
        got, fallbacks = e.run_text()
        assert fallbacks == 0 and got.count(b"\n") > 3000
        return (got,)
    s1, s2, std, ext = e.run()
    return s1.tobytes(), s2.tobytes(), std.tobytes(), ext.tobytes()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_failing_sink_leaves_nothing_behind(inputs, monkeypatch, route):
    env, text, un_called = ROUTES[route]
    monkeypatch.setenv("NGSLD_TEST_BATCH_PAIRS", "500")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fresh = _prepared(inputs, text, un_called)
    try:
        want = _ordinary(fresh, text)
        if un_called:
            assert fresh.replay_info()["sites_degenerate"] * 64 >= N_SITES      # (what sends text through run_grouped)
    finally:
        fresh.close()

    e = _prepared(inputs, text, un_called)
    try:
        calls = [0]

        def sink(_user, _batch):
            calls[0] += 1
            return 1 if calls[0] == 3 else 0

        cb = capi.SINK_FN(sink)
        rc = e._L.ngsld_run(e._h, 0, N_SITES, cb, None)
        assert rc == capi.ERR_SINK
        assert calls[0] == 3
        assert e._L.ngsld_last_error(e._h).decode() == "sink callback failed"
        got = _ordinary(e, text)
    finally:
        e.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w) and g == w
