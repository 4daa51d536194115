"""What the edge loops of a burst of K addNewObstacle calls cost a host-pointer caller on a C4-shaped mirror (the graph
of tools/bench_graph.py: 200 k nodes, both directed edges between nodes closer than the ball radius), measured in one
process:

  (a) singles  K x rrtx_obstacle_sweep, then ONE rrtx_graph_edges_block over all the ids they returned.  Existing API
               only, so this leg also runs on an older build (--only-a).
  (b) batch    one rrtx_obstacle_sweep_batch(block = 1).

The obstacles are the first K of the first 64 spheres of synth.spheres(256), range robotRadius + delta + radius.  Host
clocks around synchronous calls, the legs alternated call by call so that both see the same machine, every leg warmed
up first.  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_sweep_batch.py [--steps 300] [--warmup 30] [--out profiles/sweep_batch_c4.json] [--only-a]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true", help="time leg (a) alone (a build without the batched call)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.nodes
    pts = synth.nodes(n, 3)
    sph = synth.spheres(256)[:64]
    search = RR + DELTA + sph[:, 3]
    res = dict(n_nodes=n, steps=args.steps, warmup=args.warmup, robot_radius=RR, delta=DELTA)
    with Context(3, node_capacity=n) as ctx:
        ctx.nodes_append(pts)
        s, e = build_edges(ctx, pts, synth.ball_radius(n, 3))
        ctx.graph_edges_append(s, e)
        ctx.spheres_set(sph)
        res["n_edges"] = int(len(s))
        for K in (1, 8, 64):
            pos = np.arange(K, dtype=np.int32)
            first = [ctx.obstacle_sweep(j, float(search[j]), RR, cap=1 << 20) for j in range(K)]
            total = sum(len(f) for f in first)
            cap = total + 64                          # every call of either leg fits at once: no second call is timed

            def singles():
                rows = [ctx.obstacle_sweep(j, float(search[j]), RR, cap=cap) for j in range(K)]
                ctx.graph_edges_block(np.concatenate(rows))
                return rows

            legs = {"singles_then_block": singles}
            if not args.only_a:
                legs["batch_block"] = lambda: ctx.obstacle_sweep_batch(pos, search[:K], RR, block=True, cap=cap)
                off, ids = legs["batch_block"]()
                assert np.array_equal(ids, np.concatenate(first)) and off[-1] == total
            times = {name: [] for name in legs}
            for it in range(args.warmup + args.steps):
                for name, fn in legs.items():        # alternate the legs call by call
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if it >= args.warmup:
                        times[name].append(dt)
            res[f"K{K}"] = dict(ids=int(total), **{name: summary(t) for name, t in times.items()})
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
