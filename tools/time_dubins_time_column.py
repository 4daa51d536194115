"""What RRTX_OPT_DUBINS_TIME_COLUMN costs the fused Dubins preamble: rrtx_extend_candidates_dubins_dev on the scene of
bench.py's C5 path (N = 500 k nodes in [x y t theta], theta wrapped, 256 polygons of which a quarter move in time,
velocity bounds set) at a batch that finishes in seconds, with the piecewise time column (value 0) and the reference's
running sum (value 1) ALTERNATED call by call, so that both see the same machine.  HIP events on the context's stream
around every call; median with p10-p90.  Prints one JSON line and writes it.

    python tools/time_dubins_time_column.py [--batch 1024] [--steps 60] [--warmup 6] [--out profiles/dubins_time_column_c5.json]
    python tools/time_dubins_time_column.py --only-piecewise     # a build without the option: value 0 alone,
                                                                 # profiles/dubins_time_column_c5_parent.json

The comparison that counts: the piecewise median of this build against the p10-p90 band of the --only-piecewise run
of the parent build (the run-to-run spread is the only margin), and what the running sum adds."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime image per process)

from rrtqx_3d_amd import synth  # noqa: E402
from rrtqx_3d_amd.context import Context  # noqa: E402

OPT_TIME_COLUMN = 16           # RRTX_OPT_DUBINS_TIME_COLUMN (by number: --only-piecewise runs on builds without the name)
ROBOT_RADIUS = 0.5


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=60, help="timed calls per value of the option")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-piecewise", action="store_true", help="value 0 alone, the option never touched (parent build)")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed calls per value")
    assert torch.cuda.is_available(), "needs a GPU"
    out_path = args.out or os.path.join(ROOT, "profiles", "dubins_time_column_c5_parent.json" if args.only_piecewise
                                        else "dubins_time_column_c5.json")
    cfg = synth.CONFIGS["C5"]
    N, M, B = cfg.n_nodes, cfg.n_obstacles, args.batch
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    r_min = synth.R_MIN_TIME
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(M)
    act = np.array(active, dtype=np.uint8).copy()
    act[hidden] = 1
    res = dict(config="C5", n_nodes=N, n_obstacles=M, moving=int(sum(k in (6, 7) for k in kinds)), batch=B, r=r,
               steps=args.steps, warmup=args.warmup, only_piecewise=bool(args.only_piecewise))
    dev = torch.device("cuda", 0)
    values = [0] if args.only_piecewise else [0, 1]
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(synth.V_MIN, synth.V_MAX)
        ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
        ctx.nodes_append(synth.nodes_time(N))
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            cap = 3400 * B
            t = lambda m, dt: torch.empty(m, dtype=dt, device=dev)
            dq = torch.from_numpy(synth.nodes_time(B, seed=synth.SEED + 1)).to(dev)
            off, idx = t(B + 1, torch.int64), t(cap, torch.int32)
            key, co, ci = t(cap, torch.float64), t(cap, torch.float64), t(cap, torch.float64)
            ho, hi, un, need = t(cap, torch.uint8), t(cap, torch.uint8), t(B, torch.uint8), torch.zeros(1, dtype=torch.int64, device=dev)
            ni, nd = t(B, torch.int32), t(B, torch.float64)
            st.synchronize()

            def call(value):
                if not args.only_piecewise:
                    ctx.set_option(OPT_TIME_COLUMN, value)
                ctx.extend_candidates_dubins_dev(dq.data_ptr(), B, r, ROBOT_RADIUS, r_min, off.data_ptr(), idx.data_ptr(),
                                                 key.data_ptr(), co.data_ptr(), ci.data_ptr(), None, None, ho.data_ptr(),
                                                 hi.data_ptr(), cap, need.data_ptr(), ni.data_ptr(), nd.data_ptr(), un.data_ptr())

            hits = {}
            for _ in range(args.warmup):
                for v in values:
                    call(v)
            st.synchronize()
            ev = {v: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                  for v in values}
            for it in range(args.steps):
                for v in values:                             # alternate the two values call by call
                    e0, e1 = ev[v][it]
                    e0.record(st); call(v); e1.record(st)
            st.synchronize()
            n = int(need.item())
            assert 0 < n <= cap, (n, cap)
            for v in values:                                 # what the two forms answer on this scene
                call(v)
                st.synchronize()
                hits[v] = (int((ho[:n] & 1).sum().item()), int((hi[:n] & 1).sum().item()))
        ctx.set_stream(None)
    res["neighbours"] = n
    names = {0: "piecewise", 1: "running_sum"}
    for v in values:
        res[names[v]] = summary([e0.elapsed_time(e1) for e0, e1 in ev[v]])
        res[names[v]]["collisions_out_in"] = hits[v]
    if not args.only_piecewise:
        res["running_sum_over_piecewise"] = res["running_sum"]["median_ms"] / res["piecewise"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
