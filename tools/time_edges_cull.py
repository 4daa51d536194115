"""What rrtx_graph_edges_cull / rrtx_graph_edges_compact cost, and what a compacted mirror saves the calls that stream it,
on a mirror grown by the C4 law (N = 200 000 uniform nodes in the 100^3 world, gamma = 80, delta = 8: i <-> j, i < j,
linked when |p_i - p_j| < min(delta, gamma (ln(1 + j) / j)^(1/3)); edge order is extend()'s).  One process, one job:

  1. per repetition, on a mirror appended afresh and solved once: cull of every node at the final ball; the
     rrtx_graph_cost_update that follows; rrtx_graph_edges_compact.
  2. on the compacted mirror and on an uncompacted twin (same cull, same update, no compaction), alternately call by
     call: rrtx_graph_cost_to_root; rrtx_graph_cost_update with nothing new; rrtx_obstacle_sweep_batch of 8 spheres.

Every call is clocked twice: HIP events recorded on the context's stream either side of it, and the host clock (the
calls end synchronised).  Medians with p10 - p90 after the warm-up repetitions; the bytes the marking and compaction
passes move are computed from the edge counts.  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_edges_cull.py [--nodes 200000] [--reps 7] [--steps 30] [--out profiles/edges_cull.json]
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

GAMMA, DELTA, RR, ROOT = 80.0, 8.0, 0.5, 0


def ball(n):
    return min(DELTA, GAMMA * (math.log(1 + n) / n) ** (1.0 / 3.0))


def grow_edges(ctx, pts, chunk=16384):
    """Appends the nodes to the (empty) context chunk by chunk and returns both directed edges of every pair the law
    links, in extend()'s order: for j ascending and its neighbours i < j ascending, j -> i then i -> j"""
    n = len(pts)
    s, e = [], []
    for a in range(0, n, chunk):
        j = np.arange(a, min(a + chunk, n))
        ctx.nodes_append(pts[j])                        # the tree a node of the chunk can see: no node beyond the chunk
        r = np.array([ball(max(int(x), 1)) for x in j])
        off, idx, _ = ctx.nn_radius(pts[j], r)
        own = np.repeat(j, np.diff(off))
        keep = idx < own
        own, idx = own[keep].astype(np.int32), idx[keep].astype(np.int32)
        pair = np.empty((len(own), 2), dtype=np.int32)
        pair[:, 0], pair[:, 1] = own, idx
        s.append(pair.reshape(-1))
        pair = np.empty((len(own), 2), dtype=np.int32)
        pair[:, 0], pair[:, 1] = idx, own
        e.append(pair.reshape(-1))
    return np.concatenate(s), np.concatenate(e)


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


class Clock:
    """HIP events on the context's stream and the host clock around one call"""

    def __init__(self, ctx):
        self.stream = torch.cuda.ExternalStream(ctx.get_stream())

    def __call__(self, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        t0 = time.perf_counter()
        out = fn()
        host = (time.perf_counter() - t0) * 1e3
        b.record(self.stream)
        b.synchronize()
        return out, a.elapsed_time(b), host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    n = args.nodes
    pts = synth.nodes(n, 3)
    r = ball(n)
    res = dict(n_nodes=n, ball=r, gamma=GAMMA, delta=DELTA, reps=args.reps, warmup=args.warmup, steps=args.steps)
    with Context(3, node_capacity=n) as ctx, Context(3, node_capacity=n) as twin:
        twin.nodes_append(pts)
        s, e = grow_edges(ctx, pts)
        ne = int(len(s))
        res["n_edges"] = ne
        clock, clock_twin = Clock(ctx), Clock(twin)
        ev = {k: [] for k in ("cull", "update_after_cull", "compact")}
        host = {k: [] for k in ev}
        culled = removed = 0
        remap = None
        for rep in range(args.warmup + args.reps):
            ctx.graph_edges_clear()
            ctx.graph_edges_append(s, e)
            ctx.graph_cost_to_root(ROOT)
            (culled), t_e, t_h = clock(lambda: ctx.graph_edges_cull(r))
            steps = [("cull", t_e, t_h)]
            _, t_e, t_h = clock(lambda: ctx.graph_cost_update(ROOT))
            steps.append(("update_after_cull", t_e, t_h))
            (remap, removed), t_e, t_h = clock(lambda: ctx.graph_edges_compact())
            steps.append(("compact", t_e, t_h))
            if rep >= args.warmup:
                for k, a, b in steps:
                    ev[k].append(a); host[k].append(b)
        assert removed == culled
        left = ne - removed
        res.update(culled=int(culled), share_culled=culled / ne, edges_left=left)
        res["events"] = {k: summary(v) for k, v in ev.items()}
        res["host_clock"] = {k: summary(v) for k, v in host.items()}
        # bytes: mark reads start and end of every edge, dist and the culled byte of those with start < end, and writes
        # dist, dist0, dirty, culled of the culled ones; compaction reads the culled byte twice and the five columns of
        # every survivor (25 B), writes them and remap
        current = int((s < e).sum())
        res["current_out_edges"] = current
        res["bytes"] = dict(mark=8 * ne + 9 * current + 18 * culled, compact=2 * ne + 50 * left + 4 * ne)
        res["gb_per_s"] = dict(mark=res["bytes"]["mark"] / res["events"]["cull"]["median_ms"] / 1e6,
                               compact=res["bytes"]["compact"] / res["events"]["compact"]["median_ms"] / 1e6)
        # the twin: the same cull and update, no compaction
        twin.graph_edges_append(s, e)
        twin.graph_cost_to_root(ROOT)
        assert twin.graph_edges_cull(r) == culled
        twin.graph_cost_update(ROOT)
        rng = np.random.default_rng(8)
        sph = np.concatenate([rng.uniform(-0.8 * synth.WORLD, 0.8 * synth.WORLD, (8, 3)), np.full((8, 1), 5.0)], 1)
        for c in (ctx, twin):
            c.spheres_set(sph, np.ones(8, dtype=np.uint8))
        calls = {"cost_to_root": lambda c: c.graph_cost_to_root(ROOT),
                 "update_nothing_new": lambda c: c.graph_cost_update(ROOT),
                 "sweep_batch_8": lambda c: c.obstacle_sweep_batch(list(range(8)), RR + DELTA + 5.0, RR, cap=1 << 20)}
        legs = {"compacted": (ctx, clock), "uncompacted": (twin, clock_twin)}
        times = {name: {leg: [] for leg in legs} for name in calls}
        same = {}
        for it in range(5 + args.steps):
            for name, fn in calls.items():
                outs = {}
                for leg, (c, ck) in legs.items():
                    out, t_e, _ = ck(lambda: fn(c))
                    outs[leg] = out
                    if it >= 5:
                        times[name][leg].append(t_e)
                if it == 0:
                    a, b = outs["compacted"], outs["uncompacted"]
                    if name != "sweep_batch_8":
                        same[name] = bool(np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)))
                    else:
                        # the twin still lists the culled ids (they are blocked edges to a sweep): its rows are longer.
                        # The same rows once its ids go through remap and the removed ones are dropped.
                        rows_b = [remap[b[1][b[0][j]:b[0][j + 1]]] for j in range(8)]
                        rows_b = [r[r >= 0] for r in rows_b]
                        rows_a = [a[1][a[0][j]:a[0][j + 1]] for j in range(8)]
                        same[name + "_through_remap"] = bool(all(np.array_equal(x, y) for x, y in zip(rows_a, rows_b)))
                        res["sweep_batch_8_ids"] = dict(compacted=int(len(a[1])), uncompacted=int(len(b[1])))
        res["same_result"] = same
        res["alternated"] = {name: {leg: summary(v) for leg, v in t.items()} for name, t in times.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
