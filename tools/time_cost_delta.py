"""What a replanning step's cost update costs a host-pointer caller who wants rrtLMC on the device for the next
rrtx_extend_select / rrtx_find_new_target, on a C4-shaped mirror (the graph of tools/bench_graph.py: 200 k nodes, both
directed edges between nodes closer than the ball radius, root = node 0), measured in one process:

  (a) today's caller  rrtx_graph_cost_update with both full arrays, then rrtx_node_cost_set of all nodes.
  (b) delta           one rrtx_graph_cost_update_delta(store = 1), room for every node offered (no second call).

Scenario: the edges one sphere sweeps are blocked and unblocked in turn (rrtx_graph_edges_block / _unblock, outside the
clock), and the update after every switch is timed.  Two placements of the sphere: next to the root (the worst case of
DESIGN 4.7: a large part of the tree hangs below the blocked edges) and near the corner of the world farthest from the
root (few nodes change).  Each leg has a context of its own over the same graph, so both see the same switch every
time and neither solves on the other's behalf; the legs are alternated call by call.  Host clocks around calls that end
synchronised, every leg warmed up first; median with p10 - p90, and the number of nodes that change per placement and
direction.  --only-a times leg (a) alone (a build without the delta call).  Prints one JSON line and, with --out FILE,
writes it.

    python tools/time_cost_delta.py [--steps 300] [--warmup 30] [--only-a] [--out profiles/cost_delta_c4.json]
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

RR, RADIUS, ROOT = 0.5, 5.0, 0


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
    ap.add_argument("--only-a", action="store_true", help="time leg (a) alone (a build without the delta call)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.nodes
    pts = synth.nodes(n, 3)
    r = synth.ball_radius(n, 3)
    corner = -np.sign(pts[ROOT]) * (synth.WORLD - RADIUS)
    placements = {"root": np.array([pts[ROOT, 0] + 6.0, pts[ROOT, 1], pts[ROOT, 2], RADIUS]),
                  "corner": np.array([corner[0], corner[1], corner[2], RADIUS])}
    res = dict(n_nodes=n, steps=args.steps, warmup=args.warmup, robot_radius=RR, sphere_radius=RADIUS, only_a=args.only_a)
    names = ["full_arrays_then_node_cost_set"] + ([] if args.only_a else ["delta_store"])
    ctxs = {name: Context(3, node_capacity=n) for name in names}
    try:
        s = e = None
        for ctx in ctxs.values():
            ctx.nodes_append(pts)
            if s is None:
                s, e = build_edges(ctx, pts, r)
            ctx.graph_edges_append(s, e)
        res["n_edges"] = int(len(s))

        update_ms = []                                # rrtx_graph_cost_update's share of leg (a), call by call

        def leg_a():
            ctx = ctxs[names[0]]
            t0 = time.perf_counter()
            lmc, par, _ = ctx.graph_cost_update(ROOT)
            update_ms.append((time.perf_counter() - t0) * 1e3)
            ctx.node_cost_set(0, lmc)
            return lmc, par

        def leg_b():
            return ctxs["delta_store"].graph_cost_update_delta(ROOT, store=True, cap=n)
        legs = {names[0]: leg_a}
        if not args.only_a:
            legs["delta_store"] = leg_b
        for place, sph in placements.items():
            for ctx in ctxs.values():
                ctx.spheres_set(sph[None, :], np.ones(1, dtype=np.uint8))
            ids = ctxs[names[0]].obstacle_sweep(0, RR + r + RADIUS, RR, cap=1 << 20)
            for fn in legs.values():                  # the state before the sphere; (b)'s first call reports every node
                fn()
            prev = leg_a()
            changed, times = {}, {name: {"block": [], "unblock": []} for name in legs}
            times["graph_cost_update_alone"] = {"block": [], "unblock": []}
            for it in range(args.warmup + args.steps):
                way = "block" if it % 2 == 0 else "unblock"
                for ctx in ctxs.values():             # outside the clock: every leg sees the same switch
                    (ctx.graph_edges_block if way == "block" else ctx.graph_edges_unblock)(ids)
                for name, fn in legs.items():         # alternate the legs call by call
                    t0 = time.perf_counter()
                    out = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if it >= args.warmup:
                        times[name][way].append(dt)
                        if name == names[0]:
                            times["graph_cost_update_alone"][way].append(update_ms[-1])
                    if name == names[0]:              # the nodes that change: (a) by comparing its arrays, (b) as reported
                        k = int(((out[0].view(np.uint64) != prev[0].view(np.uint64)) | (out[1] != prev[1])).sum())
                        prev = out
                    else:
                        k = int(len(out[0]))
                    if it < 2:
                        changed.setdefault(way, {})[name] = k
            for way in changed:
                assert len(set(changed[way].values())) == 1, ("the legs disagree on the changed nodes", place, changed)
            res[place] = dict(sphere=sph.tolist(), blocked_edges=int(len(ids)),
                              changed_nodes={way: next(iter(v.values())) for way, v in changed.items()},
                              **{name: dict(all=summary(t["block"] + t["unblock"]), block=summary(t["block"]),
                                            unblock=summary(t["unblock"])) for name, t in times.items()})
    finally:
        for ctx in ctxs.values():
            ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
