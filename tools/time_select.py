"""What one extend step costs a host-pointer caller at C4 (N = 200k, M = 256, B = 16384), with and without the
selection step on the device, measured in one process:

  (a) extend_candidates  rrtx_extend_candidates with host pointers: every neighbour with cost and both flags comes back
                         (~414 k entries x 14 bytes).  Existing API only, so this leg also runs on an older build.
  (b) extend_select      rrtx_extend_select with host pointers, rrtLMC set once with rrtx_node_cost_set: the per-sample
                         block and the rewire lists come back.
  (c) select_dev         rrtx_extend_select_dev alone over lists already on the device, by HIP events around the call
                         (three launches), next to the extend step it follows (events around rrtx_extend_candidates_dev).

(a) and (b) are host clocks around synchronous calls, alternated step by step so that both see the same machine; every
leg is warmed up first.  Prints one JSON line and, with --out FILE, writes it.

    python tools/time_select.py [--steps 300] [--warmup 30] [--out profiles/select_c4.json] [--only-a]
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


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true", help="time leg (a) alone (a build without the selection step)")
    args = ap.parse_args()
    if args.steps < 200:
        ap.error("--steps: at least 200 timed steps per leg")
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C4"]
    N, M, B = cfg.n_nodes, cfg.n_obstacles, cfg.batch
    r = synth.ball_radius(N, 3)
    Q = synth.queries(B, 3)
    rng = np.random.default_rng(1)
    lmc = rng.uniform(0.0, 60.0, N)                  # a tree whose costs do not follow its geometry: many rewire entries
    lmc[rng.random(N) < 0.05] = np.inf
    lmc[0] = 0.0
    res = dict(config="C4", n_nodes=N, n_obstacles=M, batch=B, r=r, steps=args.steps, warmup=args.warmup)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(synth.nodes(N, 3))
        ctx.spheres_set(synth.spheres(M))
        first = ctx.extend_candidates(Q, r, 0.5)
        k = len(first["idx"])
        res["neighbours"] = k
        bufs_a = ctx.extend_out_buffers(B, k + 64)
        leg_a = lambda: ctx.extend_candidates(Q, r, 0.5, out=bufs_a)
        # two trees: costs that do not follow the geometry (nearly every neighbour is a rewire candidate: the most that
        # can come back) and costs within 10 % of the straight line to the root (a tree that has converged: few are)
        pts = synth.nodes(N, 3)
        line = np.sqrt(((pts - pts[0]) ** 2).sum(axis=1))
        scenarios = {"random_costs": lmc, "near_optimal_costs": line * rng.uniform(1.0, 1.1, N)}
        for sc, cost in ({"": None} if args.only_a else scenarios).items():
            legs = {"extend_candidates_host": leg_a}
            if not args.only_a:
                ctx.node_cost_set(0, cost)
                probe = ctx.extend_select(Q, r, 0.5)
                nrw_sc = len(probe["rw_node"])
                res[sc] = dict(rewire_entries=nrw_sc, ok_samples=int((probe["status"] == 0).sum()),
                               bytes_back_a=int(k * 14 + B * 21 + 8), bytes_back_b=int(nrw_sc * 12 + B * 42 + 24))
                bufs_b = ctx.select_out_buffers(B, nrw_sc + 64)
                legs["extend_select_host"] = lambda: ctx.extend_select(Q, r, 0.5, out=bufs_b)
            times = {name: [] for name in legs}
            for it in range(args.warmup + args.steps):
                for name, fn in legs.items():            # alternate the legs step by step
                    t0 = time.perf_counter()
                    fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    if it >= args.warmup:
                        times[name].append(dt)
            for name in legs:
                (res[sc] if sc else res)[name] = summary(times[name])
        if not args.only_a:
            ctx.node_cost_set(0, lmc)
            nrw = res["random_costs"]["rewire_entries"]
        if not args.only_a:
            # (c) the device-form selection alone, and the extend step before it, by events on the context's stream
            dev = torch.device("cuda", 0)
            st = torch.cuda.Stream(device=dev)
            ctx.set_stream(st.cuda_stream)
            with torch.cuda.stream(st):
                cap = k + 64
                t = lambda m, dt: torch.empty(m, dtype=dt, device=dev)
                dq, d_lmc = torch.from_numpy(Q).to(dev), torch.from_numpy(lmc).to(dev)
                off, idx, cost = t(B + 1, torch.int64), t(cap, torch.int32), t(cap, torch.float64)
                ho, hi, un, need = t(cap, torch.uint8), t(cap, torch.uint8), t(B, torch.uint8), t(1, torch.int64)
                ni, nd = t(B, torch.int32), t(B, torch.float64)
                pi, pe, ln, stt = t(B, torch.int32), t(B, torch.int64), t(B, torch.float64), t(B, torch.uint8)
                rwo, rwn, rwv, rwneed = t(B + 1, torch.int64), t(nrw + 64, torch.int32), t(nrw + 64, torch.float64), t(1, torch.int64)
                st.synchronize()
                extend = lambda: ctx.extend_candidates_dev(dq.data_ptr(), B, r, 0.5, off.data_ptr(), idx.data_ptr(), cost.data_ptr(),
                                                           ho.data_ptr(), hi.data_ptr(), cap, need.data_ptr(), ni.data_ptr(),
                                                           nd.data_ptr(), un.data_ptr())
                select = lambda: ctx.extend_select_dev(B, off.data_ptr(), idx.data_ptr(), cost.data_ptr(), cost.data_ptr(),
                                                       ho.data_ptr(), hi.data_ptr(), need.data_ptr(), cap, un.data_ptr(),
                                                       d_lmc.data_ptr(), pi.data_ptr(), pe.data_ptr(), ln.data_ptr(), stt.data_ptr(),
                                                       rwo.data_ptr(), rwn.data_ptr(), rwv.data_ptr(), nrw + 64, rwneed.data_ptr())
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
                for _ in range(args.warmup):
                    extend(); select()
                st.synchronize()
                for e0, e1, e2 in ev:
                    e0.record(st); extend(); e1.record(st); select(); e2.record(st)
                st.synchronize()
                assert int(rwneed.item()) == nrw and int(need.item()) == k
            ctx.set_stream(None)
            res["extend_dev_events"] = summary([e0.elapsed_time(e1) for e0, e1, _ in ev])
            res["select_dev_events"] = summary([e1.elapsed_time(e2) for _, e1, e2 in ev])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
