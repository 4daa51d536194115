"""What the lists of a Dubins batch's samples among themselves cost beside the Dubins extend step, on the C3 scene
(N = 50k nodes in [x y t theta], 64 polygons, theta wrapped, r = 10, r_min = 1) with B = 1024 and B = 4096 samples, in
one process, by HIP events on the context's stream:

  (a) extend       around rrtx_extend_candidates_dubins_dev alone;
  (b) extend+self  around that call followed by rrtx_extend_candidates_self_dubins_dev on the same batch (skip = the
                   sample_unsafe bytes the first call left on the device).

The legs alternate step by step, so both see the same machine; both are warmed up first.  Recorded per batch size: the
entries of both lists, median / p10 / p90 of both legs and the difference of the medians.  Prints one JSON line and,
with --out FILE, writes it.  --kernels-only B runs leg (b) alone, without events, for a separate
`rocprofv3 --kernel-trace --stats` run that gives the per-kernel split.

    python tools/time_extend_self_dubins.py [--steps 200] [--warmup 20] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (before the library: one HIP runtime image per process)

from rrtqx_3d_amd import synth  # noqa: E402
from rrtqx_3d_amd.context import Context  # noqa: E402

RR, RMIN, R = 0.5, 1.0, 10.0


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--kernels-only", type=int, default=0, metavar="B", help="leg (b) alone at batch size B, no events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 200 and not args.kernels_only:
        ap.error("--steps: at least 200 timed steps per leg")
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C3"]
    N, M = cfg.n_nodes, cfg.n_obstacles
    res = dict(config="C3", n_nodes=N, n_obstacles=M, r=R, r_min=RMIN, robot_radius=RR, steps=args.steps,
               warmup=args.warmup, batches={})
    dev = torch.device("cuda", 0)
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(synth.nodes(N, 4))
        ctx.polygons_set(synth.polygons(M))
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            for B in ([args.kernels_only] if args.kernels_only else args.batches):
                Q = synth.queries(B, 4)
                t = lambda m, dt: torch.empty(m, dtype=dt, device=dev)
                dq = torch.from_numpy(Q).to(dev)
                need, need_s, un = t(1, torch.int64), t(1, torch.int64), t(B, torch.uint8)
                off, off_s, ni, nd = t(B + 1, torch.int64), t(B + 1, torch.int64), t(B, torch.int32), t(B, torch.float64)

                def lists(cap):
                    return (t(cap, torch.int32), t(cap, torch.float64), t(cap, torch.float64), t(cap, torch.float64),
                            t(cap, torch.uint8), t(cap, torch.uint8))
                # the two counts first, then room for both lists
                cap, cap_s = 512 * B, 8 * B
                for _ in range(2):
                    idx, key, co, ci, ho, hi = lists(cap)
                    idx_s, key_s, co_s, ci_s, ho_s, hi_s = lists(cap_s)
                    st.synchronize()
                    extend = lambda: ctx.extend_candidates_dubins_dev(
                        dq.data_ptr(), B, R, RR, RMIN, off.data_ptr(), idx.data_ptr(), key.data_ptr(), co.data_ptr(),
                        ci.data_ptr(), None, None, ho.data_ptr(), hi.data_ptr(), cap, need.data_ptr(), ni.data_ptr(),
                        nd.data_ptr(), un.data_ptr())
                    self_ = lambda: ctx.extend_candidates_self_dubins_dev(
                        dq.data_ptr(), B, R, RR, RMIN, un.data_ptr(), off_s.data_ptr(), idx_s.data_ptr(), key_s.data_ptr(),
                        co_s.data_ptr(), ci_s.data_ptr(), None, None, ho_s.data_ptr(), hi_s.data_ptr(), cap_s,
                        need_s.data_ptr())
                    extend(); self_()
                    st.synchronize()
                    k, k_s = int(need.item()), int(need_s.item())
                    if k <= cap and k_s <= cap_s:
                        break
                    cap, cap_s = max(cap, k + 64), max(cap_s, k_s + 64)
                assert k <= cap and k_s <= cap_s
                if args.kernels_only:
                    for _ in range(args.warmup + args.steps):
                        extend(); self_()
                    st.synchronize()
                    continue
                ev_a = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)]
                ev_b = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)]
                for _ in range(args.warmup):
                    extend(); extend(); self_()
                st.synchronize()
                for (a0, a1), (b0, b1) in zip(ev_a, ev_b):          # the legs alternate step by step
                    a0.record(st); extend(); a1.record(st)
                    b0.record(st); extend(); self_(); b1.record(st)
                st.synchronize()
                assert int(need.item()) == k and int(need_s.item()) == k_s
                leg_a = summary([e0.elapsed_time(e1) for e0, e1 in ev_a])
                leg_b = summary([e0.elapsed_time(e1) for e0, e1 in ev_b])
                res["batches"][str(B)] = dict(batch=B, tree_entries=k, self_entries=k_s, unsafe_samples=int(un.sum().item()),
                                              pair_tests=B * (B - 1) // 2, extend_events=leg_a, extend_self_events=leg_b,
                                              self_median_ms=leg_b["median_ms"] - leg_a["median_ms"])
        ctx.set_stream(None)
    if args.kernels_only:
        return
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
