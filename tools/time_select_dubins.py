"""What one Dubins extend batch costs on the C3 scene (N = 50k, M = 64 polygons, theta wrapped) at B = 1024 and 4096, the
way it had to be done before and with the lists staying on the device, measured in one process on one build:

  (a) host_fed   rrtx_extend_candidates_dubins with host pointers (every neighbour with its key, both costs and both
                 flags comes back; findBestParent on the host is left out), rrtx_nodes_append of the accepted samples,
                 rrtx_graph_edges_append_lists of the fetched lists.
  (b) linked     rrtx_extend_select_dubins (rrtLMC on the device), rrtx_nodes_append of the samples it accepted, and
                 rrtx_graph_edges_append_selected: nothing but the per-sample block and node_of crosses the bus.
  (c) alone      rrtx_extend_select_dubins by itself, in a loop of its own after the alternated one, in the same
                 process: held against its clock inside leg (b).

(a) and (b) are host clocks around synchronous calls, alternated step by step so that both see the same machine, each
leg clocked as a whole and call by call; every leg is warmed up first.  Steady state: the mirror is cleared between
steps (outside the timed region, its arrays keep their size), and the accepted samples go to a second context of the
same tree that is replaced every 16 steps (outside the timed region), so that the searched tree stays at N nodes;
node_of then names existing nodes.  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_select_dubins.py [--steps 200] [--warmup 20] [--out profiles/select_dubins.json]
"""
import argparse
import ctypes as C
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

RR, R_MIN = 0.5, 1.0
LISTS = ("offsets", "idx", "cost_out", "cost_in", "hit_out", "hit_in")


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def run_batch(ctx, pts, Q, r, steps, warmup):
    N, B = len(pts), len(Q)
    probe = ctx.extend_select_dubins(Q, r, RR, R_MIN, want_lists=True)
    k = len(probe["idx"])
    ins = probe["status"] == 0
    node_of = np.full(B, -1, dtype=np.int32)
    node_of[ins] = np.arange(int(ins.sum()), dtype=np.int32)          # existing nodes stand in (see the docstring)
    Qin = np.ascontiguousarray(Q[ins])
    # the linked append gives the mirror the host-fed one gives
    _, edges, _ = ctx.graph_edges_append_selected(node_of)
    linked = ctx.graph_edges_get()
    ctx.graph_edges_clear()
    ctx.graph_edges_append_lists(*[probe[n] for n in LISTS], node_of)
    fed = ctx.graph_edges_get()
    ctx.graph_edges_clear()
    for x, y in zip(linked, fed):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    res = dict(batch=B, neighbours=k, inserted=int(ins.sum()), edges=int(edges),
               blocked_out_edges=int((probe["hit_out"][np.repeat(ins, np.diff(probe["offsets"]))] != 0).sum()),
               bytes_a=int(Q.nbytes + k * 30 + B * 21 + 8 + Qin.nbytes + k * 22 + B * 12 + 8 + 24), bytes_b=int(Q.nbytes + B * 42 + 24 + B * 4 + Qin.nbytes + 24))
    # leg (a) calls the C entry point over arrays allocated once; leg (b) the binding with out= (no allocation either)
    cap = k + 64
    a = dict(offsets=np.empty(B + 1, np.int64), idx=np.empty(cap, np.int32), key=np.empty(cap), cost_out=np.empty(cap),
             cost_in=np.empty(cap), hit_out=np.empty(cap, np.uint8), hit_in=np.empty(cap, np.uint8),
             nearest_idx=np.empty(B, np.int32), nearest_dist=np.empty(B), sample_unsafe=np.empty(B, np.uint8))
    p = {n: v.ctypes.data for n, v in a.items()}
    bufs_b = ctx.select_out_buffers(B, len(probe["rw_node"]) + 64, dubins=True)
    sink = [None]

    def new_sink():
        if sink[0] is not None:
            sink[0].close()
        sink[0] = Context(4, node_capacity=N + 34 * B)
        sink[0].set_wrap(3, 2.0 * math.pi)
        sink[0].nodes_append(pts)

    parts = {n: [] for n in ("host_fed_candidates", "host_fed_nodes_append", "host_fed_append_lists", "linked_select",
                             "linked_nodes_append", "linked_append_selected")}

    def leg_a():
        needed = C.c_int64()
        t0 = time.perf_counter()
        rc = ctx._lib.rrtx_extend_candidates_dubins(ctx.handle, Q.ctypes.data, B, r, RR, R_MIN, p["offsets"], p["idx"], p["key"],
                                                    p["cost_out"], p["cost_in"], None, None, p["hit_out"], p["hit_in"], cap,
                                                    C.byref(needed), p["nearest_idx"], p["nearest_dist"], p["sample_unsafe"])
        ctx._check(rc)
        t1 = time.perf_counter()
        sink[0].nodes_append(Qin)
        t2 = time.perf_counter()
        n = int(needed.value)
        ctx.graph_edges_append_lists(a["offsets"], a["idx"][:n], a["cost_out"][:n], a["cost_in"][:n], a["hit_out"][:n],
                                     a["hit_in"][:n], node_of, want_rows=False)
        t3 = time.perf_counter()
        return ("host_fed_candidates", t1 - t0), ("host_fed_nodes_append", t2 - t1), ("host_fed_append_lists", t3 - t2)

    def leg_b():
        t0 = time.perf_counter()
        ctx.extend_select_dubins(Q, r, RR, R_MIN, out=bufs_b)
        t1 = time.perf_counter()
        sink[0].nodes_append(Qin)
        t2 = time.perf_counter()
        ctx.graph_edges_append_selected(node_of, want_rows=False)
        t3 = time.perf_counter()
        return ("linked_select", t1 - t0), ("linked_nodes_append", t2 - t1), ("linked_append_selected", t3 - t2)

    legs = {"host_fed": leg_a, "linked": leg_b}
    times = {name: [] for name in legs}
    for it in range(warmup + steps):
        if it % 16 == 0:
            new_sink()
        for name, fn in legs.items():                    # alternate the legs step by step
            t0 = time.perf_counter()
            split = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= warmup:
                times[name].append(dt)
                for part, d in split:
                    parts[part].append(d * 1e3)
            assert ctx.n_graph_edges == edges
            ctx.graph_edges_clear()
    sink[0].close()
    alone = []
    for it in range(warmup + steps):                     # (c) the select call by itself
        t0 = time.perf_counter()
        ctx.extend_select_dubins(Q, r, RR, R_MIN, out=bufs_b)
        if it >= warmup:
            alone.append((time.perf_counter() - t0) * 1e3)
    for name in legs:
        res[name] = summary(times[name])
    for name in parts:
        res[name] = summary(parts[name])
    res["select_alone"] = summary(alone)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="1024,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C3"]
    N, M = cfg.n_nodes, cfg.n_obstacles
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)       # R/dubinsExperimentsForPaper.jl:102
    pts, polys = synth.nodes(N, 4), synth.polygons(M)
    line = np.sqrt(((pts[:, :2] - pts[0, :2]) ** 2).sum(axis=1))
    lmc = line * np.random.default_rng(1).uniform(1.0, 1.1, N)      # a tree that has converged
    res = dict(config="C3", n_nodes=N, n_obstacles=M, r=r, r_min=R_MIN, steps=args.steps, warmup=args.warmup, runs=[])
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.polygons_set(polys)
        ctx.nodes_append(pts)
        ctx.node_cost_set(0, lmc)
        for B in (int(b) for b in args.batches.split(",")):
            res["runs"].append(run_batch(ctx, pts, synth.queries(B, 4), r, args.steps, args.warmup))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
