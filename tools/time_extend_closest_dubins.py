"""What rrtx_extend_closest_self_dubins (the k nearest earlier samples of a Dubins batch in the wrapped space, for the
closestNode rule) costs on the C3 scene (N = 50k nodes in [x y t theta], 64 polygons, theta wrapped, r = 10, r_min = 1)
with B = 1024 and B = 4096 samples and k = 8, in one process, by HIP events on the context's stream.  Three legs of the
call, which differ in `want` alone:

  (none)  want all zero: the late phase of a run, no tree list is empty;
  (tenth) 10 % of the samples wanted;
  (all)   every sample wanted;

and, in the same run, the extend step (rrtx_extend_candidates_dubins_dev) and the self call
(rrtx_extend_candidates_self_dubins_dev) each on its own.  skip = the sample_unsafe bytes and tree_idx = the nearest_idx
the extend call left on the device.  The five legs alternate step by step, so all see the same machine; all are warmed
up first.  Recorded per batch size: median / p10 / p90 of every leg, the rows filled and the slots used per leg.  Prints
one JSON line and, with --out FILE, writes it.  --kernels-only LEG --batches B runs one leg of the call alone, without
events, for a separate `rocprofv3 --kernel-trace --stats` run.

    python tools/time_extend_closest_dubins.py [--steps 200] [--warmup 20] [--out profiles/extend_closest_dubins.json]
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
LEGS = ("none", "tenth", "all")


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--kernels-only", default=None, choices=LEGS, help="one leg of the call alone, no events")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 200 and not args.kernels_only:
        ap.error("--steps: at least 200 timed steps per leg")
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C3"]
    N, M, k = cfg.n_nodes, cfg.n_obstacles, args.k
    res = dict(config="C3", n_nodes=N, n_obstacles=M, r=R, r_min=RMIN, robot_radius=RR, k=k, steps=args.steps,
               warmup=args.warmup, batches={})
    dev = torch.device("cuda", 0)
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(synth.nodes(N, 4))
        ctx.polygons_set(synth.polygons(M))
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            for B in args.batches:
                Q = synth.queries(B, 4)
                t = lambda m, dt: torch.empty(m, dtype=dt, device=dev)
                dq = torch.from_numpy(Q).to(dev)
                need, need_s, un = t(1, torch.int64), t(1, torch.int64), t(B, torch.uint8)
                off, off_s, ni, nd = t(B + 1, torch.int64), t(B + 1, torch.int64), t(B, torch.int32), t(B, torch.float64)
                rng = np.random.default_rng(5)
                want = dict(none=torch.zeros(B, dtype=torch.uint8, device=dev),
                            tenth=torch.from_numpy((rng.random(B) < 0.1).astype(np.uint8)).to(dev),
                            all=torch.ones(B, dtype=torch.uint8, device=dev))
                c_idx, c_cnt = t(B * k, torch.int32), t(B, torch.int32)
                c_key, c_co, c_ci = (t(B * k, torch.float64) for _ in range(3))
                c_ho, c_hi = t(B * k, torch.uint8), t(B * k, torch.uint8)
                c_tco, c_tci, c_tho, c_thi = t(B, torch.float64), t(B, torch.float64), t(B, torch.uint8), t(B, torch.uint8)

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
                    n_tree, n_self = int(need.item()), int(need_s.item())
                    if n_tree <= cap and n_self <= cap_s:
                        break
                    cap, cap_s = max(cap, n_tree + 64), max(cap_s, n_self + 64)
                assert n_tree <= cap and n_self <= cap_s

                def closest(leg):
                    ctx.extend_closest_self_dubins_dev(
                        dq.data_ptr(), B, k, RR, RMIN, un.data_ptr(), want[leg].data_ptr(), ni.data_ptr(), c_idx.data_ptr(),
                        c_key.data_ptr(), c_co.data_ptr(), c_ci.data_ptr(), None, None, c_ho.data_ptr(), c_hi.data_ptr(),
                        c_cnt.data_ptr(), c_tco.data_ptr(), c_tci.data_ptr(), None, None, c_tho.data_ptr(), c_thi.data_ptr())
                if args.kernels_only:
                    for _ in range(args.warmup + args.steps):
                        closest(args.kernels_only)
                    st.synchronize()
                    continue
                names = ("extend", "self") + LEGS
                calls = dict(extend=extend, self=self_, **{leg: (lambda leg=leg: closest(leg)) for leg in LEGS})
                filled = {}
                for leg in LEGS:
                    closest(leg)
                    st.synchronize()
                    filled[leg] = dict(rows=int((c_cnt > 0).sum().item()), slots=int(c_cnt.sum().item()),
                                       blocked_out=int((c_ho != 0).sum().item()), blocked_in=int((c_hi != 0).sum().item()),
                                       tree_blocked_out=int((c_tho != 0).sum().item()))
                ev = {n: [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)] for n in names}
                for _ in range(args.warmup):
                    for n in names:
                        calls[n]()
                st.synchronize()
                for s in range(args.steps):                      # the legs alternate step by step
                    for n in names:
                        e0, e1 = ev[n][s]
                        e0.record(st); calls[n](); e1.record(st)
                st.synchronize()
                res["batches"][str(B)] = dict(
                    batch=B, tree_entries=n_tree, self_entries=n_self, unsafe_samples=int(un.sum().item()),
                    pair_tests=B * (B - 1) // 2, filled=filled,
                    events={n: summary([e0.elapsed_time(e1) for e0, e1 in ev[n]]) for n in names})
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
