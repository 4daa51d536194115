"""What one call of a host-pointer extend entry point costs the caller, destinations kept across calls in pageable numpy
arrays (what context.py hands the library): a host clock around the call, which returns after its last transfer.

  3-D, the C4 scene (N = 200k, M = 256 spheres), B = 16 384:   candidates, candidates_self, closest_self (k = 8)
  Dubins, the C3 scene (N = 50k, 64 polygons, theta wrapped, r = 10, r_min = 1), B = 1024 and 4096:
                                                               candidates_self_dubins, closest_self_dubins (k = 8)

(rrtx_extend_candidates_dubins is not timed: its host form is not on the shared staging path)

One run times the library of one tree (--root, default this one) and writes one JSON file.  Two builds are compared by
running them in turn, several rounds each, inside one job, and then

    python tools/time_extend_host.py --compare NEW_1.json NEW_2.json ... --against OLD_1.json OLD_2.json ... --out FILE

which records per call the median of every round, each build's spread over its rounds (largest minus smallest round
median) and whether the new build is slower than the old by more than the larger spread.

    python tools/time_extend_host.py [--root DIR] [--steps 100] [--warmup 10] --out FILE
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

RR, RMIN, R4, K = 0.5, 1.0, 10.0, 8
I4, F8, U1 = np.int32, np.float64, np.uint8


def summary(us):
    a = np.sort(np.asarray(us, dtype=np.float64))
    q = lambda p: float(a[min(len(a) - 1, int(p * len(a)))])
    return dict(n=len(a), median_us=q(0.5), p10_us=q(0.1), p90_us=q(0.9))


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    us = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        us.append(1e6 * (time.perf_counter() - t0))
    return summary(us)


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    from rrtqx_3d_amd import _capi, synth
    from rrtqx_3d_amd.context import Context
    p = _capi._ptr
    res = dict(steps=args.steps, warmup=args.warmup, calls={})

    def csr(ctx, fn, head, words, tail=()):
        """a two-call entry point: the count with no room first, then arrays of exactly that room, kept"""
        B = head[1]
        off, need = np.empty(B + 1, dtype=np.int64), C.c_int64()
        cols = 3 if words else 1
        null = [None] * (3 + cols + (2 if words else 0))
        fn(ctx.handle, *head, p(off), *null, 0, C.byref(need), *tail)
        cap = int(need.value)
        arrays = [np.empty(cap, I4)] + [np.empty(cap, F8) for _ in range(cols)] + \
                 ([np.empty((cap, 3), U1), np.empty((cap, 3), U1)] if words else []) + [np.empty(cap, U1), np.empty(cap, U1)]
        return cap, (lambda: fn(ctx.handle, *head, p(off), *[p(a) for a in arrays], cap, C.byref(need), *tail))

    def record(name, B, entries, call):
        assert call() == _capi.RRTX_OK, name
        res["calls"][f"{name} B={B}"] = dict(entries=entries, **timed(call, args.warmup, args.steps))

    cfg = synth.CONFIGS["C4"]
    B = cfg.batch
    with Context(3, node_capacity=cfg.n_nodes) as ctx:
        ctx.nodes_append(synth.nodes(cfg.n_nodes, 3))
        ctx.spheres_set(synth.spheres(cfg.n_obstacles))
        lib, Q, r = ctx._lib, synth.queries(B, 3), synth.ball_radius(cfg.n_nodes, 3)
        skip = (np.random.default_rng(1).random(B) < 0.1).astype(U1)
        ni, nd, un = np.empty(B, I4), np.empty(B, F8), np.empty(B, U1)
        cap, call = csr(ctx, lib.rrtx_extend_candidates, (p(Q), B, r, RR), False, (p(ni), p(nd), p(un)))
        record("candidates", B, cap, call)
        cap, call = csr(ctx, lib.rrtx_extend_candidates_self, (p(Q), B, r, RR, p(skip)), False)
        record("candidates_self", B, cap, call)
        idx, cost, ho, hi = np.empty((B, K), I4), np.empty((B, K), F8), np.empty((B, K), U1), np.empty((B, K), U1)
        cnt, tho, thi = np.empty(B, I4), np.empty(B, U1), np.empty(B, U1)
        tree = np.random.default_rng(2).integers(0, cfg.n_nodes, B).astype(I4)
        record("closest_self", B, B * K, lambda: lib.rrtx_extend_closest_self(
            ctx.handle, p(Q), B, K, RR, p(skip), None, p(tree), p(idx), p(cost), p(ho), p(hi), p(cnt), p(tho), p(thi)))

    cfg = synth.CONFIGS["C3"]
    with Context(4, node_capacity=cfg.n_nodes) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(synth.nodes(cfg.n_nodes, 4))
        ctx.polygons_set(synth.polygons(cfg.n_obstacles))
        lib = ctx._lib
        for B in (1024, 4096):
            Q = synth.queries(B, 4)
            skip = (np.random.default_rng(1).random(B) < 0.1).astype(U1)
            cap, call = csr(ctx, lib.rrtx_extend_candidates_self_dubins, (p(Q), B, R4, RR, RMIN, p(skip)), True)
            record("candidates_self_dubins", B, cap, call)
            idx, ho, hi = np.empty((B, K), I4), np.empty((B, K), U1), np.empty((B, K), U1)
            key, co, ci = np.empty((B, K), F8), np.empty((B, K), F8), np.empty((B, K), F8)
            wo, wi = np.empty((B, K, 3), U1), np.empty((B, K, 3), U1)
            cnt, tco, tci = np.empty(B, I4), np.empty(B, F8), np.empty(B, F8)
            two, twi, tho, thi = np.empty((B, 3), U1), np.empty((B, 3), U1), np.empty(B, U1), np.empty(B, U1)
            tree = np.random.default_rng(2).integers(0, cfg.n_nodes, B).astype(I4)
            record("closest_self_dubins", B, B * K, lambda: lib.rrtx_extend_closest_self_dubins(
                ctx.handle, p(Q), B, K, RR, RMIN, p(skip), None, p(tree), p(idx), p(key), p(co), p(ci), p(wo), p(wi), p(ho),
                p(hi), p(cnt), p(tco), p(tci), p(two), p(twi), p(tho), p(thi)))
    return res


def compare(new_files, old_files):
    load = lambda files: [json.load(open(f))["calls"] for f in files]
    new, old = load(new_files), load(old_files)
    out = dict(rounds=dict(new=len(new), parent=len(old)), unit="us per call, host clock", calls={})
    for name in new[0]:
        n, o = [r[name]["median_us"] for r in new], [r[name]["median_us"] for r in old]
        spread = max(max(n) - min(n), max(o) - min(o))
        out["calls"][name] = dict(entries=new[0][name]["entries"], new_round_medians=n, parent_round_medians=o,
                                  new_median=float(np.median(n)), parent_median=float(np.median(o)), larger_spread=spread,
                                  slower_beyond_spread=bool(np.median(n) - np.median(o) > spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--compare", nargs="+", default=None, metavar="NEW.json")
    ap.add_argument("--against", nargs="+", default=None, metavar="OLD.json")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = compare(args.compare, args.against) if args.compare else measure(args)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
