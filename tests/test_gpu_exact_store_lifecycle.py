"""GPU: the two transitions of the exact store's life that a context walks between runs (exact_store.h: ExactStore::stop and
ExactStore::reset; the store itself is held by test_gpu_replay_lkl.py).

A new replay SOURCE drops the store -- the next run that wants one builds it again -- and leaves a failure standing; a new
MATRIX drops the store and the failure with it.  Both on 300 sites x 60 individuals of un-called input, every pair's EM in the
pair kernel (NGSLD_REPLAY_SKIP=0, as the `eng` fixture of test_gpu_replay_lkl.py), so that host-replay and device-replay runs
compare record by record."""
import pytest

from ngsld_amd import capi
from test_gpu_replay_lkl import assert_same_records, run_records, uncalled
from util import close

pytestmark = pytest.mark.gpu

N_SITES, N_IND = 300, 60


@pytest.fixture()
def eng(monkeypatch):
    monkeypatch.setenv("NGSLD_REPLAY_SKIP", "0")   # (read at ngsld_create)
    e = capi.Engine(0)
    yield e
    e.close()


def test_a_new_source_drops_the_store_and_the_next_run_builds_it_again(eng):
    raw = uncalled(N_SITES, N_IND, seed=88, mono_frac=0.3)
    host = run_records(eng, raw, 0)
    first = run_records(eng, raw, 2)
    assert first[4]["exact_store"] == 2 and first[4]["exact_store_build_s"] > 0 and first[4]["pairs_on_device"] > 0
    eng.set_replay_source(raw)                   # the same values, registered again: the store was built from the old source
    assert eng.replay_info()["exact_store"] == 0
    n = eng.plan()
    s1, s2, std, ext = eng.run()
    again = (s1, s2, std.copy(), ext.copy(), eng.replay_info())
    assert len(s1) == n == len(first[0])
    assert again[4]["exact_store"] == 2 and again[4]["pairs_on_device"] == first[4]["pairs_on_device"] > 0
    assert_same_records(first, again)
    assert_same_records(host, again)


def test_a_new_matrix_clears_a_failed_store(eng, monkeypatch):
    raw = uncalled(N_SITES, N_IND, seed=88, mono_frac=0.3)
    monkeypatch.setenv("NGSLD_TEST_EXACT_STORE_NO_ROOM", "1")
    host = run_records(eng, raw, 2)              # no room: the flagged pairs are the host's
    assert host[4]["exact_store"] == 0 and host[4]["pairs_on_device"] == 0 and host[4]["pairs_on_host"] > 0
    monkeypatch.delenv("NGSLD_TEST_EXACT_STORE_NO_ROOM")
    dev = run_records(eng, raw, 2)               # set_geno_raw again on the same engine: a new matrix, a new try
    assert dev[4]["exact_store"] == 2 and dev[4]["pairs_on_device"] > 0
    assert dev[4]["pairs_replayed"] == host[4]["pairs_replayed"]
    assert close(dev[2]["r2_ExpG"], host[2]["r2_ExpG"]).all()
    for col in dev[2].dtype.names:
        if col != "r2_ExpG":
            assert dev[2][col].tobytes() == host[2][col].tobytes(), col
    assert dev[3].tobytes() == host[3].tobytes()
