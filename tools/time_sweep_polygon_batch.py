"""What the edge loops of a burst of k addNewObstacle calls of the POLYGON list cost a host-pointer caller, measured in
one process on two scenes:

  c5      the scene of bench.py --config C5: DubinsEdge in [x y t theta], 500 k nodes (synth.nodes_time), 256 polygons
          of which a quarter move in time (synth.dynamic_polygons), the mirror of both directed edges of every pair of
          nodes within 2.0; the burst is the first k moving obstacles.  Unlike the bench scene every polygon is in use
          from the start (the bench keeps the obstacles that are yet to appear out of use).
  simple  SimpleEdge in the plane (a dim = 3 tree at z = 0): 200 k nodes, the 256 polygons of synth.polygons, the
          mirror of both directed edges of every pair within 0.6; the burst is the first k polygons.

Per scene and k = 1, 2, 4, 8, 16:

  (a) singles  k x rrtx_obstacle_sweep_polygon (mode 0), then ONE rrtx_graph_edges_block over their concatenated ids:
               the path a caller has without the batched call, and the reference of the comparison.
  (b) batch    one rrtx_obstacle_sweep_polygon_batch(block = 1).

Host clocks around synchronous calls, every call with room for all its ids (no second call is timed), the legs warmed
up first.  Leg (a) is timed in five separate loops of --steps calls; max - min of their medians is the noise margin the
difference between (a) and (b) is held against.  Leg (b) is one loop of --steps calls run between the third and the
fourth loop of (a).  After the loops one more call of each leg runs with the kernel families timed by events
(device_ms_*: the sweep passes, the Dubins steering, the Dubins check), outside the clock.  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_sweep_polygon_batch.py [--scene c5|simple|both] [--steps 20] [--warmup 3]
                                             [--out profiles/sweep_polygon_batch.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the library: one HIP runtime image per process)

from rrtqx_3d_amd import synth  # noqa: E402
from rrtqx_3d_amd.context import Context  # noqa: E402

RR = 0.5
KS = (1, 2, 4, 8, 16)


def median(ms):
    return float(np.median(np.asarray(ms, dtype=np.float64)))


def mirror(ctx, pts, r_graph):
    es_l, ee_l = [], []
    n = len(pts)
    for a in range(0, n, 32768):
        b = min(n, a + 32768)
        off, idx, _ = ctx.nn_radius(pts[a:b], r_graph, cap=64 * (b - a))
        own = np.repeat(np.arange(a, b, dtype=np.int32), np.diff(off))
        keep = own != idx
        es_l.append(own[keep]); ee_l.append(idx[keep])
    es, ee = np.concatenate(es_l), np.concatenate(ee_l).astype(np.int32)
    ctx.graph_edges_append(es, ee)
    return len(es)


def scene_c5(n):
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(256)
    ctx = Context(4, node_capacity=n)
    ctx.set_wrap(3, 2.0 * math.pi)
    ctx.set_space_has_time(True)
    ctx.set_dubins_velocity(synth.V_MIN, synth.V_MAX)
    ctx.polygons_set(polys, kinds=kinds, paths=paths, active=np.ones(len(polys), dtype=np.uint8))
    pts = synth.nodes_time(n)
    ctx.nodes_append(pts)
    ne = mirror(ctx, pts, 2.0)
    burst = [j for j in range(len(polys)) if kinds[j] in (6, 7)][:max(KS)]
    return ctx, dict(n_nodes=n, n_edges=ne, delta=10.0, r_min=synth.R_MIN_TIME), burst


def scene_simple(n):
    polys = synth.polygons(256)
    ctx = Context(3, node_capacity=n)
    ctx.polygons_set(polys)
    pts = synth.nodes(n, 3)
    pts[:, 2] = 0.0
    ctx.nodes_append(pts)
    ne = mirror(ctx, pts, 0.6)
    return ctx, dict(n_nodes=n, n_edges=ne, delta=8.0, r_min=0.0), list(range(max(KS)))


def measure(ctx, info, burst, steps, warmup):
    delta, r_min = info["delta"], info["r_min"]
    out = dict(info)
    for k in KS:
        pos = np.array(burst[:k], dtype=np.int32)
        first = [ctx.obstacle_sweep_polygon(int(p), RR, delta, r_min=r_min, cap=1 << 22) for p in pos]
        total = sum(len(f) for f in first)
        cap = total + 64

        def singles():
            rows = [ctx.obstacle_sweep_polygon(int(p), RR, delta, r_min=r_min, cap=cap) for p in pos]
            ids = np.concatenate(rows)                    # (block takes an id twice: no union is formed on the host)
            if len(ids):
                ctx.graph_edges_block(ids)

        def batch():
            return ctx.obstacle_sweep_polygon_batch(pos, RR, delta, r_min=r_min, block=True, cap=cap)

        off, ids = batch()
        assert np.array_equal(ids, np.concatenate(first)) and off[-1] == total
        cand = int(ctx.stats().last_sweep_candidates)

        def loop(fn):
            ms = []
            for it in range(warmup + steps):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if it >= warmup:
                    ms.append(dt)
            return median(ms)

        a = [loop(singles) for _ in range(3)]
        b = loop(batch)
        a += [loop(singles) for _ in range(2)]
        # where the device time goes, outside the clock: one more call of each leg with the kernel families timed by events
        # (sweep passes and tail | Dubins steering | Dubins check)
        def families(fn):
            ctx.profile(2)
            s0 = ctx.stats()
            before = (s0.ms_edges, s0.ms_dubins_steer, s0.ms_dubins)
            fn()
            s1 = ctx.stats()
            ctx.profile(0)
            return dict(zip(("sweep_ms", "dubins_steer_ms", "dubins_check_ms"),
                            (s1.ms_edges - before[0], s1.ms_dubins_steer - before[1], s1.ms_dubins - before[2])))

        out[f"k{k}"] = dict(ids=int(total), batch_candidates=cand, singles_then_block_median_ms=a,
                            singles_then_block_ms=median(a), noise_margin_ms=max(a) - min(a), batch_block_median_ms=b,
                            device_ms_singles=families(singles), device_ms_batch=families(batch))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="both", choices=("c5", "simple", "both"))
    ap.add_argument("--nodes-c5", type=int, default=synth.CONFIGS["C5"].n_nodes)
    ap.add_argument("--nodes-simple", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(steps=args.steps, warmup=args.warmup, robot_radius=RR)
    for name, make, n in (("c5", scene_c5, args.nodes_c5), ("simple", scene_simple, args.nodes_simple)):
        if args.scene in (name, "both"):
            ctx, info, burst = make(n)
            with ctx:
                res[name] = measure(ctx, info, burst, args.steps, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
