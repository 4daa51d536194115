"""What feeding the edge mirror with one extend batch costs at C4 (N = 200k, M = 256, B = 16384), the way it had to be
done before and with the lists staying on the device, measured in one process on one build:

  (a) host_fed   rrtx_extend_candidates with host pointers (every neighbour with cost and both flags comes back), the
                 start / end arrays built with numpy (vectorised: repeat, cumsum, scatter), rrtx_graph_edges_append of
                 them and rrtx_graph_edges_block of the out-edges whose flag is set.
  (b) linked     rrtx_extend_select (rrtLMC on the device), rrtx_nodes_append of the samples it accepted, and
                 rrtx_graph_edges_append_selected: nothing but the per-sample block and node_of crosses the bus.
  (c) kernels    rrtx_graph_edges_append_lists_dev alone over lists already on the device, by HIP events around the call
                 (count, scan, the 24-byte read-back, fill); the kernels by themselves are in the rocprofv3 trace
                 (--trace-only runs a short loop of this leg for `rocprofv3 --kernel-trace --stats`).

(a) and (b) are host clocks around synchronous calls, alternated step by step so that both see the same machine; every
leg is warmed up first.  Steady state: the mirror is cleared between steps (outside the timed region, its arrays keep
their size), and the accepted samples of leg (b) go to a second context of the same tree that is replaced every 16 steps
(outside the timed region), so that the searched tree stays at N nodes; node_of then names existing nodes.  Prints one
JSON line and, with --out FILE, writes it.

    python tools/time_edges_append_lists.py [--steps 300] [--warmup 30] [--out profiles/edges_append_lists.json]
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

RR = 0.5


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def build_edges(lists, node_of):
    """The order rule of rrtx_graph_edges_append_lists, vectorised: (start, end, positions of the blocked out-edges)."""
    owner = np.repeat(np.arange(len(node_of)), np.diff(lists["offsets"]))
    v = node_of[owner]
    keep = v >= 0
    v, u = v[keep], lists["idx"][keep]
    both = lists["hit_in"][keep] == 0
    cnt = 1 + both.astype(np.int64)
    pos = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    start, end = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
    start[pos], end[pos] = v, u
    start[pos[both] + 1], end[pos[both] + 1] = u[both], v[both]
    return start, end, pos[lists["hit_out"][keep] != 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="a short loop of leg (c) alone, for the kernel trace")
    args = ap.parse_args()
    if args.steps < 200 and not args.trace_only:
        ap.error("--steps: at least 200 timed steps per leg")
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C4"]
    N, M, B = cfg.n_nodes, cfg.n_obstacles, cfg.batch
    r = synth.ball_radius(N, 3)
    pts, sph, Q = synth.nodes(N, 3), synth.spheres(M), synth.queries(B, 3)
    line = np.sqrt(((pts - pts[0]) ** 2).sum(axis=1))
    lmc = line * np.random.default_rng(1).uniform(1.0, 1.1, N)      # a tree that has converged
    res = dict(config="C4", n_nodes=N, n_obstacles=M, batch=B, r=r, steps=args.steps, warmup=args.warmup)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        ctx.node_cost_set(0, lmc)
        probe = ctx.extend_select(Q, r, RR, want_lists=True)
        k = len(probe["idx"])
        ins = probe["status"] == 0
        node_of = np.full(B, -1, dtype=np.int32)
        node_of[ins] = np.arange(int(ins.sum()), dtype=np.int32)      # existing nodes stand in (see the docstring)
        Qin = np.ascontiguousarray(Q[ins])
        start, end, blocked = build_edges(probe, node_of)
        res.update(neighbours=k, inserted=int(ins.sum()), edges=len(start), blocked_out_edges=len(blocked),
                   bytes_a=int(k * 14 + B * 21 + 8 + len(start) * 8 + len(blocked) * 4), bytes_b=int(B * 42 + 24 + B * 4 + Qin.nbytes + 24))
        # the linked append gives the mirror the host-fed one gives (costs by set_dist left out of (a), as specified)
        ctx.graph_edges_append_selected(node_of)
        got = ctx.graph_edges_get()
        assert np.array_equal(got[0], start) and np.array_equal(got[1], end) and np.array_equal(np.nonzero(np.isinf(got[2]))[0], blocked)
        ctx.graph_edges_clear()
        if not args.trace_only:
            bufs_a = ctx.extend_out_buffers(B, k + 64)
            bufs_b = ctx.select_out_buffers(B, len(probe["rw_node"]) + 64)
            sink = [None]

            def new_sink():
                if sink[0] is not None:
                    sink[0].close()
                sink[0] = Context(3, node_capacity=N + 17 * B)
                sink[0].nodes_append(pts)

            def leg_a():
                lists = ctx.extend_candidates(Q, r, RR, out=bufs_a)
                s, e, b = build_edges(lists, node_of)
                first = ctx.graph_edges_append(s, e)
                ctx.graph_edges_block((first + b).astype(np.int32))

            parts = {"linked_select": [], "linked_nodes_append": [], "linked_append_selected": []}

            def leg_b():                                  # (its three calls are also clocked one by one)
                t0 = time.perf_counter()
                ctx.extend_select(Q, r, RR, out=bufs_b)
                t1 = time.perf_counter()
                sink[0].nodes_append(Qin)
                t2 = time.perf_counter()
                ctx.graph_edges_append_selected(node_of, want_rows=False)
                t3 = time.perf_counter()
                for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                    parts[name].append(dt * 1e3)

            legs = {"host_fed": leg_a, "linked": leg_b}
            times = {name: [] for name in legs}
            for it in range(args.warmup + args.steps):
                if it % 16 == 0:
                    new_sink()
                for name, fn in legs.items():            # alternate the legs step by step
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if it >= args.warmup:
                        times[name].append(dt)
                    assert ctx.n_graph_edges == len(start)
                    ctx.graph_edges_clear()
            sink[0].close()
            for name in legs:
                res[name] = summary(times[name])
            for name in parts:
                res[name] = summary(parts[name][args.warmup:])
        # (c) the device form alone over lists on the device, by events on the context's stream
        dev = torch.device("cuda", 0)
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        n_c = 40 if args.trace_only else args.steps
        with torch.cuda.stream(st):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            off, idx, cost, ho, hi = up(probe["offsets"]), up(probe["idx"]), up(probe["cost"]), up(probe["hit_out"]), up(probe["hit_in"])
            need, d_node = torch.tensor([k], dtype=torch.int64, device=dev), up(node_of)
            st.synchronize()
            link = lambda: ctx.graph_edges_append_lists_dev(B, off.data_ptr(), idx.data_ptr(), cost.data_ptr(), cost.data_ptr(),
                                                            ho.data_ptr(), hi.data_ptr(), need.data_ptr(), k, d_node.data_ptr())
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(n_c)]
            for _ in range(min(args.warmup, 10)):
                link(); ctx.graph_edges_clear()
            st.synchronize()
            for e0, e1 in ev:
                e0.record(st); first, added = link(); e1.record(st)
                assert added == len(start)
                ctx.graph_edges_clear()
            st.synchronize()
        ctx.set_stream(None)
        res["append_lists_dev_events"] = summary([e0.elapsed_time(e1) for e0, e1 in ev])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
