"""bench.py on the GPU: a plain run prints the headline line only, and --dump-outputs writes what the LAST timed step
returned (batch (steps - 1) % RING of the fresh-batch ring), checked here against the CPU oracle on a few samples."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rrtqx_3d_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_step(oracle, tmp_path):
    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["unit"] == "edges/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0
    for k in ("cpu_baseline", "roofline", "kernel_ms", "steady_state", "large_batch", "host_buffer_path"):
        assert k not in line, k                 # side measurements only with --full

    d = {n[:-4]: np.load(os.path.join(str(tmp_path), n)) for n in os.listdir(str(tmp_path))}
    assert set(d) == {"offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe"}
    assert all(a.dtype == np.float64 for a in d.values())
    cfg = synth.CONFIGS["C4"]
    N, B = cfg.n_nodes, cfg.batch
    off = d["offsets"].astype(np.int64)
    k = int(off[-1])
    assert off.shape == (B + 1,) and off[0] == 0 and np.all(np.diff(off) >= 0)
    assert d["idx"].shape == (k,) and d["cost"].shape == (k,) and d["hit_out"].shape == (k,) and d["hit_in"].shape == (k,)
    assert d["nearest_idx"].shape == (B,) and np.all((d["idx"] >= 0) & (d["idx"] < N))
    # the samples of the last timed step (bench.py make_mode, weak scaling, edge shard 0)
    Q = synth.queries(B, 3, seed=synth.SEED + 1 + 17 * ((steps - 1) % 8))
    pts = synth.nodes(N, 3)
    rad = synth.ball_radius(N, 3)
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    for i in np.random.default_rng(5).choice(B, 16, replace=False):
        ri, rk = tree.within_range(rad, Q[i])
        o = np.argsort(ri)
        assert np.array_equal(d["idx"][off[i]:off[i + 1]], ri[o].astype(np.float64)), f"neighbour set of sample {i}"
        assert np.array_equal(d["cost"][off[i]:off[i + 1]], rk[o]), f"edge costs of sample {i}"
    # all eight arrays, every sample, against the oracle's extend() preamble of that step (C4's 256 spheres)
    ref = oracle.extend_candidates_batch(oracle.TreeSet(3, pts), Q, rad, pts, oracle.make_spheres(synth.spheres(cfg.n_obstacles)),
                                         0.5, per_sample=40)
    oracle.assert_same_results(d, ref, tuple(sorted(d)), label="bench dump: ")
    assert k > 20 * B and 0 < ref["hit_out"].sum() < k and 0 < ref["sample_unsafe"].sum() < B
    print(f"\nbench dump: {B} samples, {k} entries, all eight arrays against the oracle")
