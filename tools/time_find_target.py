"""What picking new move targets costs a host-pointer caller at C4 (N = 200k, M = 256 spheres), measured in one process:

  (a) host_loop   what a caller has to do without rrtx_find_new_target: per round rrtx_extend_candidates with host
                  pointers over the poses still searching (every neighbour with cost and both flags comes back), the
                  first minimum of rrtLMC + cost per pose in numpy, the ball doubled for the poses without one.
                  Existing API only, so this leg also runs on an older build (--only-a).
  (b) device      rrtx_find_new_target, rrtLMC set once with rrtx_node_cost_set: the lists stay on the device.

For nq = 4 (the reference's four agents) and nq = 4096, and two rrtLMC layouts: every pose resolves in round 1, and a
mix in which the balls of the first rounds hold orphans only (every node within r0 * 2^(j - 1) * 0.99 of pose i at +Inf,
j = i mod 4).  One first radius for all poses, since (a) searches with one radius per call.  Host clocks around
synchronous calls, the legs alternated call by call, every leg warmed up first; both legs must give the same targets.
Prints one JSON line and, with --out FILE, writes it.

    python tools/time_find_target.py [--steps 300] [--warmup 30] [--out profiles/find_target_c4.json] [--only-a]
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

RR, R0, R_MAX = 0.5, 2.0, 24.0


def summary(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_ms=q(0.5), p10_ms=q(0.1), p90_ms=q(0.9), min_ms=float(a[0]), max_ms=float(a[-1]))


def host_loop(ctx, poses, lmc, bufs, count=None):
    """Leg (a).  Returns (target_idx, rounds); count, a dict, receives the bytes that crossed the link."""
    nq = len(poses)
    target = np.full(nq, -1, dtype=np.int32)
    rounds = np.zeros(nq, dtype=np.int32)
    act = np.arange(nq)
    r, k = R0, 1
    up = down = 0
    while act.size:
        L = ctx.extend_candidates(poses[act], r, RR, out=bufs)
        off, idx = L["offsets"][:act.size + 1], L["idx"]
        up += act.size * 24
        down += len(idx) * 14 + act.size * 21 + 8
        with np.errstate(invalid="ignore"):
            cand = lmc[idx] + L["cost"]
        cand = np.where((L["hit_out"] == 0) & (cand < math.inf), cand, math.inf)
        rounds[act] = k
        found = np.zeros(act.size, dtype=bool)
        nz = np.flatnonzero(off[1:] > off[:-1])
        if nz.size:
            best = np.minimum.reduceat(cand, off[nz])
            owner = np.repeat(np.arange(act.size), np.diff(off))
            hit = np.flatnonzero(cand == np.repeat(best, np.diff(off)[nz]))
            first = hit[np.unique(owner[hit], return_index=True)[1]]          # the first of equal minima per pose
            first = first[cand[first] < math.inf]
            found[owner[first]] = True
            target[act[owner[first]]] = idx[first]
        r *= 2
        if r > R_MAX:
            break
        act = act[~found]
        k += 1
    if count is not None:
        count.update(bytes_up=int(up), bytes_down=int(down))
    return target, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true", help="time leg (a) alone (a build without rrtx_find_new_target)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = synth.CONFIGS["C4"]
    N, M = cfg.n_nodes, cfg.n_obstacles
    pts = synth.nodes(N, 3)
    res = dict(config="C4", n_nodes=N, n_obstacles=M, r0=R0, r_max=R_MAX, steps=args.steps, warmup=args.warmup)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(synth.spheres(M))
        for nq in (4, 4096):
            poses = synth.queries(nq, 3, seed=5)
            rng = np.random.default_rng(2)
            flat = rng.uniform(0.0, 60.0, N)
            flat[0] = 0.0
            mix = flat.copy()
            off, idx, _ = ctx.nn_radius(poses, R0 * 2.0 ** (np.arange(nq) % 4 - 1) * 0.99)
            mix[idx] = math.inf
            mix[0] = 0.0
            bufs = ctx.extend_out_buffers(nq, max(int(nq * 1500), 1 << 16))
            for layout, lmc in (("round_1", flat), ("four_round_mix", mix)):
                count = {}
                t_a, k_a = host_loop(ctx, poses, lmc, bufs, count)
                sc = dict(rounds_share=(np.bincount(k_a, minlength=5) / nq).tolist(), found=int((t_a >= 0).sum()),
                          a_bytes_up=count["bytes_up"], a_bytes_down=count["bytes_down"])
                legs = {"host_loop": lambda: host_loop(ctx, poses, lmc, bufs)}
                if not args.only_a:
                    ctx.node_cost_set(0, lmc)
                    got = ctx.find_new_target(poses, R0, R_MAX, RR)
                    assert np.array_equal(got["target_idx"], t_a) and np.array_equal(got["rounds"], k_a), (nq, layout)
                    # up: poses, radii, thresholds, slots; down: three words per round and 37 bytes per pose
                    sc.update(b_bytes_up=int(nq * (24 + 8 + 16 + 4)), b_bytes_down=int(24 * int(k_a.max()) + 37 * nq))
                    legs["find_new_target"] = lambda: ctx.find_new_target(poses, R0, R_MAX, RR)
                times = {name: [] for name in legs}
                for it in range(args.warmup + args.steps):
                    for name, fn in legs.items():            # alternate the legs call by call
                        t0 = time.perf_counter()
                        fn()
                        dt = (time.perf_counter() - t0) * 1e3
                        if it >= args.warmup:
                            times[name].append(dt)
                for name in legs:
                    sc[name] = summary(times[name])
                res[f"nq{nq}_{layout}"] = sc
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
