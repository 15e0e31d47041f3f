"""GPU, last in the suite: the cohort sizes that were cliffs in round 2's sweep, as FLOORS on this box.

Not a benchmark -- `bench.py` and `profiles/` are -- but a claim the driver's own box checks: each floor lies ABOVE what round
2's kernels reached on a fast box and 10-25 % BELOW what the round-3 kernels reach on the slowest box of the pool seen so
far (`profiles/r03/sweep_nind_r03.txt`, taken at 2.19 GHz), so a pass means the step after 512 / 640 / 2,304 / 4,608
individuals is gone here too, and a fail means a kernel selection or a register spill has regressed."""
import json
import subprocess
import sys

import pytest

from ngsld_amd import capi

pytestmark = pytest.mark.gpu

#        n_ind  floor (pairs/s)   round 2, fast box   round 3, 2.19 GHz box   kernel expected
FLOORS = [(513, 1.45e8),        # 1.20e8              1.82e8                  run kernel, nine individuals per lane
          (640, 1.30e8),        # 1.21e8              1.53e8                  run kernel, ten
          (704, 1.17e8),        # 1.13e8              1.33e8                  a/b kernel, row vector in registers
          (2560, 2.90e7),       # 2.34e7              (3.50e7, 2.3 GHz box)   four wavefronts x ten, a/b form
          (5120, 1.30e7),       # 6.2e6 (streaming)   (1.61e7, 2.3 GHz box)   eight wavefronts x ten, a/b form
          (6000, 1.05e7),       # 5.0e6 (streaming)   (1.33e7, 2.3 GHz box)   eight wavefronts x twelve, a/b form
          (10000, 3.9e6)]       # 2.6e6               (5.3e6, 2.3 GHz box)    streaming, candidate's vector in registers
KERNELS = {513: "pair_ld_run_kernel", 640: "pair_ld_run_kernel", 704: "pair_ld_ab_kernel",
           2560: "pair_ld_abm_kernel (multi-wavefront, a/b form)", 5120: "pair_ld_abm_kernel (multi-wavefront, a/b form)",
           6000: "pair_ld_abm_kernel (multi-wavefront, a/b form)",
           10000: "pair_ld_bres_kernel (streaming, candidate's vector resident)"}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n_ind,floor", FLOORS)
def test_cohort_sizes_past_the_old_cliffs_keep_their_rate(n_ind, floor):
    sites = int(max(4000, min(100000, 4e7 / n_ind)))
    cmd = [sys.executable, "bench.py", "--config", "c2", "--sites", str(sites), "--ind", str(n_ind), "--steps", "2", "--warmup", "1",
           "--no-cpu", "--no-sink", "--no-e2e", "--no-traffic"]
    r = subprocess.run(cmd, cwd=capi.REPO_DIR, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["roofline"]["kernel"] == KERNELS[n_ind], d["roofline"]["kernel"]
    print(f"\n[throughput] n_ind {n_ind}: {d['value']:.4g} pairs/s ({d['roofline']['kernel']}), floor {floor:.3g}")
    assert d["value"] >= floor, f"n_ind {n_ind}: {d['value']:.4g} pairs/s is below the floor of {floor:.3g}"


# Round 5: matrices that are NOT SNP-called (README.md:73).  With 20 % monomorphic sites a third of the pairs is flagged for the
# exact-order replay; on host threads (rounds 1-4) the pass ran at 2.2e6 pairs/s, on the device (ld_replay_lkl.hip) at 1.3e8
# (2.15e8 with the log-uniform spectrum) on a 2.2 GHz box (profiles/r05/d); 1.27e8 / 1.78e8 on the pool's slowest
# (profiles/r05/final_slow_box).  The floors were half of that; late in round 5 a hand-back test inside the lane kernel cost its
# long launches 30 % (1.30e8 -> 1.14e8) and no test saw it -- they are 15 % under the slowest box now.  (Last session of round 5:
# shared reciprocal and tiled sort key, 1.42e8 .. 1.46e8 / 2.27e8 on three boxes, profiles/r05/late/tile -- floors 1.15e8 / 1.6e8,
# still more than 15 % under what the slowest box of the pool would show.)
@pytest.mark.timeout(900)
# (Round 6: the pairs of degenerate sites skip their EM in the pair kernel, the lane replay tests its operands with one instruction,
# uses two register sets in turn and reads a copy with its rare sites first: 1.50e8 .. 1.64e8 / 2.18e8 .. 2.34e8 on the boxes of the
# round, profiles/r06 -- floors 1.35e8 / 1.9e8.)
@pytest.mark.parametrize("flags,floor", [(["--mono-frac", "0.2"], 1.35e8), (["--sfs"], 1.9e8)])
def test_uncalled_input_is_replayed_on_the_device(flags, floor):
    cmd = [sys.executable, "bench.py", "--config", "c2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu", "--no-sink",
           "--no-e2e", "--no-traffic"] + flags
    r = subprocess.run(cmd, cwd=capi.REPO_DIR, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    rep = d["config"]["replay_rank0_last_step"]
    print(f"\n[throughput] {' '.join(flags)}: {d['value']:.4g} pairs/s, {rep['pairs_flagged']} of {d['config']['pairs_per_step']} pairs "
          f"flagged, {rep['pairs_on_device']} replayed on the device, {rep['pairs_on_host']} on the host; replay off: "
          f"{d['config']['replay_off']['value']:.4g} pairs/s; first pass {d['config']['first_pass_s_rank0']} s, floor {floor:.3g}")
    assert rep["pairs_flagged"] > d["config"]["pairs_per_step"] // 30
    assert rep["pairs_on_host"] * 10_000 <= d["config"]["pairs_per_step"], "host-only share of the pairs above 1e-4"
    assert rep["pairs_on_device"] + rep["pairs_on_host"] == rep["pairs_flagged"]
    assert d["value"] >= floor, f"{flags}: {d['value']:.4g} pairs/s is below the floor of {floor:.3g}"


# Round 6: the exact store priced.  The store is the matrix once more in device memory (and once more again for the lanes'
# individual-major copy); `--max_gpu_mem` is a cap on all of it now (ngsld_set_memory_budget).  Under a budget of the fixed part + 1.5 x
# the planes -- the planes fit, planes + store + copy do not -- the binary keeps the matrix resident, builds the store, goes without
# the copy (text batches are the wavefront-per-pair kernel's anyway) and leaves next to nothing to the host's threads: 1.56 s for
# configs[2]'s un-called twin, as without a cap (profiles/r06/store_budget.json).  (Without room for the store itself the flagged
# pairs go to the host's threads at the reference's own speed: the cliff is still there below planes + store.)
@pytest.mark.timeout(900)
def test_uncalled_input_under_a_memory_budget_of_one_and_a_half_times_the_planes(tmp_path_factory):
    import os
    import re
    import tempfile
    import time

    import torch

    from ngsld_amd import shard, synth
    n_sites, n_ind = 100_000, 500
    chrs, pos = synth.make_positions(n_sites, 3)
    n_pairs = int(shard.row_pair_counts(shard.pos_dist_from_positions(chrs, pos), 100, 0).sum())
    planes_gb = n_sites * 3 * 512 * 8 / 1e9
    budget = 2.58 + 1.5 * planes_gb            # (ngsld_sites_for_budget's fixed part of one context + 1.5 x the planes)
    with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
        raw = synth.make_gl_torch(n_sites, n_ind, 3, torch.device("cuda", 0), mono_frac=0.2)
        g, p = os.path.join(d, "in.glf"), os.path.join(d, "in.pos")
        with open(g, "wb") as fh:
            for lo in range(0, n_sites, 20000):
                fh.write(raw[lo:lo + 20000].cpu().numpy().tobytes())
        del raw
        torch.cuda.empty_cache()
        synth.write_pos(p, chrs, pos)
        cmd = [capi.CLI_PATH, "--geno", g, "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--pos", p, "--max_kb_dist", "100",
               "--extend_out", "--n_threads", "16", "--verbose", "2", "--out", "/dev/null", "--max_gpu_mem", f"{budget:.2f}"]
        best, err = None, ""
        for _ in range(2):
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            best, err = (dt if best is None else min(best, dt)), r.stderr
    m = re.search(r"(\d+) of (\d+) pairs replayed .*\((\d+) on the device, (\d+) on host threads\)", err)
    assert m, err[-1500:]
    replayed, total, on_dev, on_host = (int(x) for x in m.groups())
    print(f"\n[throughput] un-called configs[2] through the binary under --max_gpu_mem {budget:.2f} GB: {best:.3f} s = {n_pairs / best:.4g} pairs/s, "
          f"{replayed} pairs replayed, {on_host} of them on host threads")
    assert total == n_pairs and replayed > n_pairs // 10 and on_dev + on_host == replayed
    assert on_host * 10_000 <= n_pairs, "host share of the pairs above 1e-4: no room was found for the exact store"
    assert n_pairs / best >= 5e7
