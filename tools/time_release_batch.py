"""What the edge loops of a burst of K corrected removeObstacle calls cost a host-pointer caller on a C4-shaped mirror
(the graph of tools/bench_graph.py: 200 k nodes, both directed edges between nodes closer than the ball radius),
measured in one process:

  (a) corrected caller  K x rrtx_obstacle_sweep, the host filter for dist == Inf (the caller's own copy of the blocked
                        set), ONE masked rrtx_edges_check_idx of the candidates against the spheres that stay, and the
                        restores: one rrtx_graph_edges_set_dist per run of consecutive freed ids.  Existing API only.
  (b) release           one rrtx_obstacle_release_batch(unblock = 1).

The sphere list is the first 64 spheres of synth.spheres(256), all in use, everything their sweeps return blocked first;
the first K of them leave, range robotRadius + delta + radius.  After every timed call the freed edges are blocked again
outside the clock, so every call of either leg sees the same mirror.  Host clocks around synchronous calls, the legs
alternated call by call so that both see the same machine, every leg warmed up first.  At K = 8 a third leg times
rrtx_obstacle_sweep_batch(block = 1), whose kernels this call leaves alone (--only-sweep-batch: that leg alone, for a
build without the release call).  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_release_batch.py [--steps 300] [--warmup 30] [--ks 1,8,64] [--out profiles/release_batch_c4.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the library: one HIP runtime image per process)

from rrtqx_3d_amd import synth  # noqa: E402
from rrtqx_3d_amd.context import Context  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_graph import build_edges  # noqa: E402

RR, DELTA = 0.5, 8.0


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-sweep-batch", action="store_true",
                    help="time rrtx_obstacle_sweep_batch(block = 1) at K = 8 alone (a build without the release call)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.nodes
    pts = synth.nodes(n, 3)
    sph = synth.spheres(256)[:64]
    M = len(sph)
    search = RR + DELTA + sph[:, 3]
    res = dict(n_nodes=n, steps=args.steps, warmup=args.warmup, robot_radius=RR, delta=DELTA)
    with Context(3, node_capacity=n) as ctx:
        ctx.nodes_append(pts)
        s, e = build_edges(ctx, pts, synth.ball_radius(n, 3))
        ctx.graph_edges_append(s, e)
        ctx.spheres_set(sph)
        res["n_edges"] = int(len(s))
        cost_host = np.sqrt(((pts[s] - pts[e]) ** 2).sum(1))           # the caller's distOriginal
        off, ids = ctx.obstacle_sweep_batch(np.arange(M, dtype=np.int32), search, RR, block=True, cap=1 << 22)
        blocked_host = np.zeros(len(s), dtype=bool)                    # the caller's copy of dist == Inf
        blocked_host[ids] = True
        res["blocked_edges"] = int(blocked_host.sum())
        pos8 = np.arange(8, dtype=np.int32)
        cap8 = int(off[8]) + 64
        sweep8 = lambda: ctx.obstacle_sweep_batch(pos8, search[:8], RR, block=True, cap=cap8)
        if args.only_sweep_batch:
            t = []
            for it in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                sweep8()
                if it >= args.warmup:
                    t.append((time.perf_counter() - t0) * 1e3)
            res["K8"] = dict(sweep_batch_block=summary(t))
        for K in ([] if args.only_sweep_batch else [int(k) for k in args.ks.split(",")]):
            pos = np.arange(K, dtype=np.int32)
            stay = np.ones(M, dtype=np.uint8)
            stay[:K] = 0
            cap = int(off[K]) + 64                    # every call of either leg fits at once: no second call is timed

            def corrected():
                rows = []
                for j in range(K):
                    r = ctx.obstacle_sweep(j, float(search[j]), RR, cap=cap)
                    rows.append(r[blocked_host[r]])
                cand = np.concatenate(rows)
                if len(cand):
                    hit, _ = ctx.edges_check_idx(s[cand], e[cand], RR, obstacle=-1, obstacle_mask=stay, want_first=False)
                    cand = cand[hit == 0]
                freed = np.unique(cand)
                if len(freed):
                    for run in np.split(freed, np.flatnonzero(np.diff(freed) != 1) + 1):
                        ctx.graph_edges_set_dist(int(run[0]), cost_host[run])
                return cand

            release = lambda: ctx.obstacle_release_batch(pos, search[:K], RR, unblock=True, cap=cap)[1]
            legs = {"corrected_caller": corrected, "release_unblock": release}
            if K == 8:
                legs["sweep_batch_block"] = lambda: sweep8()[1]
            want = release()
            freed = np.unique(want)
            ctx.graph_edges_block(freed)
            got = corrected()
            ctx.graph_edges_block(freed)
            assert np.array_equal(got, want), "the two legs free different edges"
            runs = int((np.diff(freed) != 1).sum()) + 1 if len(freed) else 0
            times = {name: [] for name in legs}
            for it in range(args.warmup + args.steps):
                for name, fn in legs.items():        # alternate the legs call by call
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    ctx.graph_edges_block(freed)     # outside the clock: the next call sees the mirror blocked again
                    if it >= args.warmup:
                        times[name].append(dt)
            res[f"K{K}"] = dict(ids=int(len(want)), freed=int(len(freed)), id_runs=runs,
                                **{name: summary(t) for name, t in times.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
