#!/usr/bin/env python3
"""Benchmark of the RRT^X extend/rewire hot path on MI355X (BASELINE.json metric).

A step = one pass of the fused extend() preamble over one batch of B synthetic
samples with every input already resident in HBM:
    radius-NN (N nodes)  ->  2*sum(k) directed SimpleEdges: cost + collision check
    against M sphere obstacles  ->  nearest + sample point check.
Every step takes a FRESH batch (a ring of pre-generated device batches), so chunk lists,
bucket histograms and cache contents differ step to step.
value = directed edges collision-checked per second (whole job, all ranks).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C4|C3|C5] [--scaling weak|strong]
                    [--obstacles spheres|polygons] [--shard edges|obstacles] [--grid ExO] [--batch B]
                    [--full] [--dump-outputs DIR]
    (--config C5: one replanning cycle of BASELINE config 5 per step, see bench_c5)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times K steps and prints the result line (value, ms_per_step, ...).  --full adds
everything else: per-kernel times and rooflines, CPU baselines, the other scaling mode, the large batch, the steady
state, the host-pointer and polygon passes.  --dump-outputs DIR writes the arrays the last timed step returned as
DIR/<name>.npy (float64; a fixed, seeded sample of each array when they exceed 64 MB together).

Multi-GPU: node SoA and obstacle list are replicated (4.8 MB and 8 KB -- trivially small next
to 288 GB of HBM).  --scaling weak (default): every rank owns its own batches of B samples.
--scaling strong: ONE global batch of B samples per step, rank r takes samples
parallel.shard_range(B, r, world).  Either way the per-edge collision bitmasks of four steps are exchanged with
one RCCL all-gather (an all-reduce over disjoint slices in an E x O grid, where one rank per obstacle group publishes)
so every rank (the planner host of every agent) sees all results.  With
N > 1 the line carries both modes (`value` is the one --scaling names, `other_scaling` the other).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP64_VALU_PEAK_TOPS = 39.3     # 78.6 TFLOP/s FMA-counted vector fp64 => 39.3 T unfused op/s
ROBOT_RADIUS = 0.5             # R/experimentsForRRTQX.jl:38
METRIC = "collision-checked edges/sec + radius-NN queries/sec at N=200k nodes, 256 obs"
RING = 8                       # pre-generated sample batches per rank
DUMP_BYTES = 60_000_000        # --dump-outputs: at most this many bytes of .npy data in all
DUMP_SEED = 20240611           # fixed seed of the sample taken of outputs larger than that


def dump_outputs(path, arrays):
    """--dump-outputs: `arrays` (name -> 1-D tensor or array, what the caller of the timed path receives) as
    path/<name>.npy in float64 (int32 / int64 indices and uint8 flags are exact in it).  Above DUMP_BYTES every array
    keeps the same fraction of its entries, chosen by DUMP_SEED: the same positions for the same lengths, run to run."""
    arrays = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).reshape(-1) for k, v in arrays.items()}
    total = 8 * sum(a.size for a in arrays.values())
    keep = min(1.0, DUMP_BYTES / max(total, 1))
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        if keep < 1.0:
            pos = np.random.default_rng(DUMP_SEED).choice(a.size, int(a.size * keep), replace=False)
            a = a[np.sort(pos)]
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float64))


def lib_sha16():
    from rrtqx_3d_amd import _capi
    with open(_capi.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def source_sha16():
    """identifies the kernel sources a committed PMC file was taken on (the .so itself is not tracked)"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "rrtqx_3d_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()[:16]


ISSUE_PEAK_GINST = 1024 * 2.4 / 4.0    # wave instructions / ns the chip can issue: 1024 SIMDs x 2.4 GHz, one per 4 cycles
                                       # whatever the type (MI355X_MICROARCH.md; measured)


def make_run_key(args, **kw):
    """what a line was measured on, beyond the kernel sources: a committed PMC file describes a line only if this
    matches (counters of another variant or workload must not ride along)"""
    k = {"config": args.config, "obstacles": args.obstacles, "batch": args.batch, "tune": args.tune, "tile_q": args.tile_q,
         "nn_cull": args.nn_cull, "nn_filter": args.nn_filter, "scan_items": args.scan_items, "scan_blocks": args.scan_blocks,
         "shard": args.shard, "grid": args.grid}
    k.update(kw)
    return k


def load_pmc(kernel, run_key):
    """the committed counters of `kernel` (profiles/r*_traffic*.json, newest round first) taken on THESE kernel
    sources and THIS run key; None otherwise.  Counters cannot be read inside this process."""
    pdir = os.path.join(ROOT, "profiles")
    src = source_sha16()
    for name in sorted((n for n in os.listdir(pdir) if n.endswith(".json") and "_traffic" in n), reverse=True):
        try:
            tj = json.load(open(os.path.join(pdir, name)))
        except (OSError, ValueError):
            continue
        if tj.get("kernel") == kernel and tj.get("source_sha16") == src and tj.get("run_key") == run_key:
            tj["file"] = "profiles/" + name
            tj["lib_match"] = tj.get("lib_sha16") == lib_sha16()
            return tj
    return None


def issue_block(tj, kernel_ms):
    """instruction-issue accounting of a kernel from its PMC passes: VALU + SALU wave instructions per launch against
    what 1024 SIMDs issue in the kernel's duration.  frac <= 1 by construction of the peak."""
    if not tj or not tj.get("SQ_INSTS_VALU_per_launch") or not kernel_ms:
        return None
    insts = tj["SQ_INSTS_VALU_per_launch"] + tj["SQ_INSTS_SALU_per_launch"]
    ach = insts / (kernel_ms * 1e6)                     # wave instructions per ns = G inst / s
    return {"valu_wave_insts_per_launch": tj["SQ_INSTS_VALU_per_launch"],
            "salu_wave_insts_per_launch": tj["SQ_INSTS_SALU_per_launch"],
            "achieved_Ginst_per_s": ach, "peak_Ginst_per_s": ISSUE_PEAK_GINST, "frac_of_kernel_time": ach / ISSUE_PEAK_GINST,
            "issue_floor_us": insts / ISSUE_PEAK_GINST * 1e-3, "wait_ratio": tj.get("wait_ratio"),
            "active_lanes_per_valu_instruction": tj.get("active_lanes_per_valu_instruction"),
            "source": tj.get("file"), "lib_match": tj.get("lib_match"),
            "note": "VALU + SALU wave instructions / (1024 SIMDs x 2.4 GHz / 4 cycles) against the kernel's duration; "
                    "wait_ratio = SQ_WAIT_ANY / SQ_WAVE_CYCLES; lanes = SQ_THREAD_CYCLES_VALU / SQ_ACTIVE_INST_VALU"}


def issue_roofline(kernel, tj, kernel_ms, extra_note=""):
    """roofline block of a kernel that instruction issue bounds (no HBM or MFMA roof applies): achieved / peak in wave
    instructions per second from the committed PMC passes; without matching passes the block says so (frac null)."""
    ib = issue_block(tj, kernel_ms)
    blk = {"kernel": kernel, "bound": "valu_issue", "unit": "Ginst/s", "peak": ISSUE_PEAK_GINST, "kernel_ms": kernel_ms,
           "achieved": ib["achieved_Ginst_per_s"] if ib else None, "frac": ib["frac_of_kernel_time"] if ib else None,
           "traffic": tj.get("traffic_bytes_per_launch") if tj else None, "traffic_unit": "bytes/launch", "issue": ib,
           "note": ("instruction-issue bound (fp64 exact tests; the obstacle table lives in LDS / L2): achieved = VALU + SALU wave "
                    "instructions per second from the PMC passes under profiles/ taken on these kernel sources and this run key"
                    if ib else "no PMC passes for these kernel sources / this run key under profiles/: achieved and frac not stated") +
                   extra_note}
    return blk


# --------------------------------------------------------------------- CPU baselines ----
def cpu_baseline(cfg, pts, Q, sph, r, budget_s=10.0, polys=None):
    """Oracle (C restatement of the reference's per-sample loop) on one host core; polys: against the polygon list."""
    from oracle import oracle as O
    tree = O.KDTree(cfg.dim)
    tree.insert_many(pts)
    if polys is not None:
        ps = O.PolygonSet(polys)
        m, what = ps.m, "polygons"
        run = lambda qs: O.extend_batch_polygons(tree, ps, qs, r, ROBOT_RADIUS)
    else:
        osph, m = O.make_spheres(sph)
        what = "spheres"
        run = lambda qs: O.extend_batch_spheres(tree, osph, m, qs, r, ROBOT_RADIUS)
    nq = Q.shape[0]
    # calibrate on a slice, then run a bounded sample
    t0 = time.perf_counter()
    run(Q[:256])
    per_q = (time.perf_counter() - t0) / 256
    n_sample = int(min(nq, max(256, budget_s / max(per_q, 1e-9))))
    t0 = time.perf_counter()
    edges, neigh, hits, _ = run(Q[:n_sample])
    dt = time.perf_counter() - t0
    out = {
        "value": edges / dt, "unit": "edges/s", "cores": 1, "kind": "port",
        "sample": f"first {n_sample} of {nq} samples of the same workload (kd-tree nearest + range + "
                  f"{edges} directed edges x {m} {what} with first-hit early-out), {dt:.1f} s on 1 host core",
        "nn_queries_per_s": n_sample / dt,
    }
    if polys is None:
        out["all_cores"] = cpu_baseline_all_cores(cfg, pts, Q, sph, r, per_q)
    return out


def cpu_baseline_all_cores(cfg, pts, Q, sph, r, per_q, budget_s=4.0):
    """The same oracle loop run embarrassingly parallel over samples, one private kd-tree per
    thread.  NOT the reference's behaviour (its loop is single-threaded, R/rrtqx.jl:947); reported
    so the GPU/CPU ratio is not read as a core-count artefact."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle as O
    try:
        n_thr = len(os.sched_getaffinity(0))
    except AttributeError:
        n_thr = os.cpu_count() or 1
    n_thr = max(1, min(n_thr, 16))
    nq = Q.shape[0]
    per_thr = int(min(nq // n_thr, max(64, budget_s / max(per_q, 1e-9))))
    osph, m = O.make_spheres(sph)

    def build(_):
        t = O.KDTree(cfg.dim)
        t.insert_many(pts)
        return t

    def run(a):
        tree, k = a
        return O.extend_batch_spheres(tree, osph, m, Q[k * per_thr:(k + 1) * per_thr], r, ROBOT_RADIUS)[0]

    with ThreadPoolExecutor(n_thr) as ex:       # ctypes calls release the GIL
        trees = list(ex.map(build, range(n_thr)))
        t0 = time.perf_counter()
        edges = sum(ex.map(run, [(trees[k], k) for k in range(n_thr)]))
        dt = time.perf_counter() - t0
    return {"value": edges / dt, "unit": "edges/s", "cores": n_thr, "kind": "port",
            "sample": f"{n_thr} threads x {per_thr} samples, private kd-tree each, {dt:.1f} s; "
                      "not the reference's (single-threaded) behaviour"}


def cpu_baseline_dubins(pts, Q, polys, r, r_min, budget_s=12.0):
    """Config 3 on one host core: the oracle's per-sample Dubins preamble (wrapped range search, both
    directed edges steered with calculateTrajectory and checked with the two-stage explicitEdgeCheck)."""
    import math
    from oracle import oracle as O
    tree = O.KDTree(4, wraps=[3], wrap_points=[2.0 * math.pi])
    tree.insert_many(pts)
    ps = O.PolygonSet(polys)
    edges, t0, n = 0, time.perf_counter(), 0
    for q in Q:
        idx, _ = tree.within_range(r, q)
        for j in idx:
            for s, g in ((q, pts[j]), (pts[j], q)):
                res = O.dubins_steer(s, g, r_min)
                O.dubins_edge_check_polygons(ps, s, g, res[-1], ROBOT_RADIUS, r_min)
                edges += 1
        n += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    return {"value": edges / dt, "unit": "edges/s", "cores": 1, "kind": "port",
            "sample": f"first {n} of {len(Q)} samples: wrapped kd-tree range search + {edges} directed Dubins edges "
                      f"steered and checked against {len(polys)} polygons, {dt:.1f} s on 1 host core",
            "nn_queries_per_s": n / dt}


# ------------------------------------------------------------------------- helpers ----
class Buffers:
    """device outputs of one fused extend() call"""

    def __init__(self, torch, dev, B, cap):
        self.off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        self.idx = torch.empty(cap, dtype=torch.int32, device=dev)
        self.cost = torch.empty(cap, dtype=torch.float64, device=dev)
        # the three flag arrays are one allocation: an obstacle-sharded run OR-reduces them in ONE all_reduce(MAX)
        self.flags = torch.zeros(2 * cap + B, dtype=torch.uint8, device=dev)
        self.hout, self.hin, self.unsafe = self.flags[:cap], self.flags[cap:2 * cap], self.flags[2 * cap:]
        self.nidx = torch.empty(B, dtype=torch.int32, device=dev)
        self.ndist = torch.empty(B, dtype=torch.float64, device=dev)
        self.cap = cap


def concurrent_agents(k, torch, dev, pts, sph, r, B, cap, N, rounds=20):
    """Side measurement, never `value`: k independent planners (the reference drives 4 agents, each
    with its own tree and obstacle list, R/rrtqx.jl:29-31) share the GPU, one context and one HIP
    stream per agent, every agent stepping its own batch."""
    from rrtqx_3d_amd import synth
    from rrtqx_3d_amd.context import Context
    agents = []
    for a in range(k):
        c = Context(3, device=dev.index or 0, node_capacity=N)
        st = torch.cuda.Stream(device=dev)
        c.set_stream(st.cuda_stream)
        c.spheres_set(sph)
        c.nodes_append(pts)
        q = torch.from_numpy(synth.queries(B, 3, seed=synth.SEED + 77 + a)).to(dev)
        agents.append((c, st, q, Buffers(torch, dev, B, cap), torch.zeros(1, dtype=torch.int64, device=dev)))

    def step(ag):
        c, st, q, b, need = ag
        c.extend_candidates_dev(q.data_ptr(), B, r, ROBOT_RADIUS, b.off.data_ptr(), b.idx.data_ptr(),
                                b.cost.data_ptr(), b.hout.data_ptr(), b.hin.data_ptr(), cap, need.data_ptr(),
                                b.nidx.data_ptr(), b.ndist.data_ptr(), b.unsafe.data_ptr())

    for _ in range(3):
        for ag in agents:
            step(ag)
    torch.cuda.synchronize()
    edges = sum(2 * int(ag[4].item()) for ag in agents)
    t0 = time.perf_counter()
    for _ in range(rounds):
        for ag in agents:
            step(ag)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for ag in agents:
        ag[0].close()
    return {"agents": k, "edges_per_s": edges * rounds / dt, "ms_per_round": 1e3 * dt / rounds,
            "note": "k contexts on k streams, each stepping its own batch of the same config; not `value`"}


def bench_c3(args, torch, dist, dev, rank, world):
    """--config C3: the fused Dubins preamble (BASELINE config 3).  Not the driver's default line."""
    import math
    from rrtqx_3d_amd import _capi, parallel, synth
    from rrtqx_3d_amd.context import Context
    cfg = synth.CONFIGS["C3"]
    N, M, B = cfg.n_nodes, cfg.n_obstacles, cfg.batch
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)       # R/dubinsExperimentsForPaper.jl:102
    r_min = 1.0
    pts, polys = synth.nodes(N, 4), synth.polygons(M)
    Q = synth.queries(B, 4, seed=synth.SEED + 1 + 1000 * rank)
    ctx = Context(4, device=dev.index or 0, node_capacity=N)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_wrap(3, 2.0 * math.pi)
    ctx.polygons_set(polys)
    ctx.nodes_append_dev(torch.from_numpy(pts).to(dev).data_ptr(), N)
    d_q = torch.from_numpy(Q).to(dev)
    cap = 2048 * B
    f64 = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device=dev)
    d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    d_idx = torch.empty(cap, dtype=torch.int32, device=dev)
    d_key, d_co, d_ci = f64(cap), f64(cap), f64(cap)
    d_ho, d_hi, d_un = u8(cap), u8(cap), u8(B)
    d_need = torch.zeros(1, dtype=torch.int64, device=dev)
    d_ni = torch.empty(B, dtype=torch.int32, device=dev)
    d_nd = f64(B)

    def compute():
        ctx.extend_candidates_dubins_dev(d_q.data_ptr(), B, r, ROBOT_RADIUS, r_min, d_off.data_ptr(), d_idx.data_ptr(),
                                         d_key.data_ptr(), d_co.data_ptr(), d_ci.data_ptr(), None, None, d_ho.data_ptr(),
                                         d_hi.data_ptr(), cap, d_need.data_ptr(), d_ni.data_ptr(), d_nd.data_ptr(),
                                         d_un.data_ptr())

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(max(args.warmup, 1)):
        compute()
    fence()
    k_total = int(d_need.item())
    if k_total > cap:
        raise SystemExit(f"candidate capacity too small: {k_total} > {cap}")
    steps = args.steps
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        compute()
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"offsets": d_off, "idx": d_idx[:k_total], "key": d_key[:k_total],
                                         "cost_out": d_co[:k_total], "cost_in": d_ci[:k_total], "hit_out": d_ho[:k_total],
                                         "hit_in": d_hi[:k_total], "nearest_idx": d_ni, "nearest_dist": d_nd,
                                         "sample_unsafe": d_un})
    if args.full:
        ctx.profile(2)
        for _ in range(2):
            compute()
        fence()
        st = ctx.stats()
        ctx.profile(0)
    e_sum, t_max = parallel.reduce_throughput(2 * k_total * steps, dt, device=dev)
    if rank == 0:
        rk = make_run_key(args)
        out = {
            "metric": METRIC, "value": e_sum / t_max, "unit": "edges/s", "n_gpus": world, "steps": steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * t_max / steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": cfg.name + " (fused Dubins preamble, wrapped theta)", "n_nodes": N, "n_obstacles": M,
                       "batch_per_gpu": B, "radius": r, "edge": "DubinsEdge", "min_turning_radius": r_min,
                       "directed_edges_per_step_per_gpu": 2 * k_total},
            "nn_queries_per_s": B * world * steps / t_max,
            "run_key": rk, "hip_runtime": _capi.hip_runtime(), "lib_sha16": lib_sha16(), "source_sha16": source_sha16(),
        }
        if args.full:
            # per step: the check launches (both directions, every chunk) and the steering launches, summed
            dub_ms = st.ms_dubins / 2
            steer_ms = st.ms_dubins_steer / 2
            chk_launches = st.launches_dubins // 2
            # Dubins steering + two-stage check is fp64 arithmetic: ~400 flops per steer plus, per
            # polyline piece that reaches stage 2, the polygon test.  The steering figure alone is a floor.
            d_kernel = "dubins_check_rec_kernel<false>"
            # the check kernel's own duration: rocprof names it; the family timer covers steer + check launches together
            tj = load_pmc(d_kernel, rk)
            if tj:      # the passes average per LAUNCH; a step is chk_launches launches of the kernel
                tj = dict(tj)
                for kk in ("SQ_INSTS_VALU_per_launch", "SQ_INSTS_SALU_per_launch", "traffic_bytes_per_launch"):
                    if tj.get(kk) is not None:
                        tj[kk] = tj[kk] * chk_launches
            out["kernel_ms"] = {"nn_scan": st.ms_nn_scan / max(st.launches_nn_scan, 1),
                                "nn_finish": st.ms_nn_finish / 2, "dubins_check": dub_ms, "dubins_steer": steer_ms,
                                "dubins_check_launches_per_step": chk_launches,
                                "points": st.ms_points / max(st.launches_points, 1)}
            out["roofline"] = issue_roofline(d_kernel, tj, dub_ms,
                                             "; kernel_ms and the instruction counts are the SUM over the check kernel's launches "
                                             "of one step (both directions, every chunk of 2 M edges); steering is a launch of its "
                                             "own (kernel_ms.dubins_steer), DESIGN.md 4.6")
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_dubins(pts, Q, polys, r, r_min)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


def cpu_baseline_c5(pts, es, ee, polys, kinds, paths, active, j_new, Q, r, r_min, rr, delta, budget_s=14.0):
    """BASELINE config 5 on one host core, bounded: the oracle's addNewObstacle edge loop for obstacle j_new
    (findPointsInConflictWithObstacle over the kd-tree, then explicitEdgeCheck(S, edge, ob) of out-edges of the nodes
    found) and the per-sample Dubins-with-time preamble of extend() (wrapped range search, both directed edges steered
    with calculateTrajectory and checked against the whole list), each until its share of the budget is spent."""
    import math
    from oracle import oracle as O
    tree = O.KDTree(4, wraps=[3], wrap_points=[2.0 * math.pi])
    tree.insert_many(pts)
    ps = O.PolygonSet(polys, kinds=kinds, paths=paths, active=active)
    t0 = time.perf_counter()
    nodes = O.points_in_conflict_polygon(tree, ps, j_new, rr, delta, True, True)
    t_query = time.perf_counter() - t0
    mark = np.zeros(len(pts), dtype=bool)
    mark[nodes] = True
    cand = np.nonzero(mark[es])[0]
    n_sw, t1 = 0, time.perf_counter()
    for e in cand:
        O.explicit_edge_check_obstacle(ps, j_new, pts[es[e]], pts[ee[e]], rr, True, r_min, has_time=True)
        n_sw += 1
        if time.perf_counter() - t1 > 0.3 * budget_s:
            break
    t_sw = time.perf_counter() - t1
    n_ex, n_q, t2 = 0, 0, time.perf_counter()
    for q in Q:
        idx, _ = tree.within_range(r, q)
        for k in idx:
            for a, b in ((q, pts[k]), (pts[k], q)):
                d, w, v, wd, tr = O.dubins_steer_time(a, b, r_min)
                if len(tr):
                    O.dubins_edge_check_polygons_time(ps, a, b, tr, rr, r_min)
                n_ex += 1
            if time.perf_counter() - t2 > 0.7 * budget_s:
                break
        n_q += 1
        if time.perf_counter() - t2 > 0.7 * budget_s:
            break
    t_ex = time.perf_counter() - t2
    return {"value": (n_sw + n_ex) / (t_sw + t_ex), "unit": "edges/s", "cores": 1, "kind": "port",
            "sample": f"obstacle {j_new} appears: kd-tree conflict query ({len(nodes)} nodes, {t_query * 1e3:.1f} ms), "
                      f"{n_sw} of {len(cand)} candidate out-edges through the two-stage Dubins check with time "
                      f"({t_sw:.1f} s); extend(): {n_ex} directed Dubins edges of the first {n_q} sample(s) steered and "
                      f"checked against {len(polys)} polygons ({t_ex:.1f} s); 1 host core",
            "sweep_edges_per_s": n_sw / max(t_sw, 1e-9), "extend_edges_per_s": n_ex / max(t_ex, 1e-9),
            "conflict_query_ms": t_query * 1e3}


def bench_c5(args, torch, dist, dev, rank, world):
    """--config C5: one REPLANNING CYCLE per step of BASELINE config 5 (DubinsEdge in [x y t theta], N = 500 k,
    256 polygons of which a quarter move in time): an obstacle appears -> rrtx_obstacle_sweep_polygon over the edge
    mirror -> rrtx_graph_edges_block -> rrtx_graph_cost_update -> the fused Dubins-with-time preamble of extend() on a
    fresh batch of 16384 samples -> the batch joins the tree.  Every rank runs its own planner (replicas, weak)."""
    import math
    from rrtqx_3d_amd import _capi, parallel, synth
    from rrtqx_3d_amd.context import Context
    cfg = synth.CONFIGS["C5"]
    N, M, B = cfg.n_nodes, cfg.n_obstacles, (args.batch or cfg.batch)
    steps, warm = args.steps, max(args.warmup, 1)
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    r_min, rr, delta = synth.R_MIN_TIME, ROBOT_RADIUS, 10.0
    pts = synth.nodes_time(N)
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(M)
    moving = [j for j in range(M) if kinds[j] in (6, 7)]
    if steps + warm > len(moving):
        raise SystemExit(f"--config C5: {steps} + {warm} cycles need that many discoverable moving obstacles, the list has {len(moving)}")
    appear = moving[:steps + warm]                     # the dynamic obstacles the robot has not seen yet, one per cycle
    act = np.array(active, dtype=np.uint8).copy()
    act[appear] = 0
    act[hidden] = 1                                    # (static ones are all known: a static obstacle cannot be swept in a
    #                                                     space with time, R/DRRT.jl:3067)
    ctx = Context(4, device=dev.index or 0, node_capacity=N + (steps + warm + 1) * B)
    stream = torch.cuda.current_stream()
    ctx.set_wrap(3, 2.0 * math.pi)
    ctx.set_space_has_time(True)
    ctx.set_dubins_velocity(synth.V_MIN, synth.V_MAX)
    ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
    ctx.nodes_append(pts)
    # ---- the planner's edge mirror: both directed edges of every pair of nodes within r_graph (the live graph of
    #      RRT^X at this size and ball radius would hold ~2 400 out-edges per node, 1.2 x 10^9 edges; the mirror here
    #      keeps the ~20 nearest, stated in the line) ----
    r_graph = 2.0
    es_l, ee_l = [], []
    for a in range(0, N, 32768):
        b = min(N, a + 32768)
        off, idx, _ = ctx.nn_radius(pts[a:b], r_graph, cap=64 * (b - a))
        own = np.repeat(np.arange(a, b, dtype=np.int32), np.diff(off))
        keep = own != idx
        es_l.append(own[keep]); ee_l.append(idx[keep])
    es, ee = np.concatenate(es_l), np.concatenate(ee_l).astype(np.int32)
    del es_l, ee_l
    ctx.graph_edges_append(es, ee)
    # edge.dist of a DubinsEdge with time.  Planning runs in reverse time: an edge leads from a later state to an earlier
    # one (validMove's first condition, R/DRRT_DubinsEdge_functions.jl:120); the velocity bounds are not applied to the
    # mirror, so that 24 out-edges per node still make a connected graph.  The root is the earliest node.
    n_valid = 0
    for a in range(0, len(es), 1 << 21):
        b = min(len(es), a + (1 << 21))
        st = ctx.dubins_steer_full(pts[es[a:b]], pts[ee[a:b]], r_min)
        ok = pts[es[a:b], 2] > pts[ee[a:b], 2]
        n_valid += int(ok.sum())
        ctx.graph_edges_set_dist(a, np.where(ok, st["dist"], np.inf))
    root = int(np.argmin(pts[:, 2]))
    lmc0, _, passes0 = ctx.graph_cost_to_root(root)
    ctx.set_stream(stream.cuda_stream)
    # ---- fresh batches and output buffers, resident before the clock starts ----
    Qs = [synth.nodes_time(B, seed=synth.SEED + 1 + 1000 * rank + 17 * j) for j in range(RING)]
    d_q = [torch.from_numpy(q).to(dev) for q in Qs]
    cap = 3400 * B
    f64 = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device=dev)
    d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    d_idx = torch.empty(cap, dtype=torch.int32, device=dev)
    d_key, d_co, d_ci = f64(cap), f64(cap), f64(cap)
    d_ho, d_hi, d_un = u8(cap), u8(cap), u8(B)
    d_need = torch.zeros(steps + warm + 1, dtype=torch.int64, device=dev)
    d_ni = torch.empty(B, dtype=torch.int32, device=dev)
    d_nd = f64(B)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    phase = {k: 0.0 for k in ("obstacle_appears", "sweep", "block", "cost_update", "extend_preamble", "append")}
    counts = {"sweep_candidates": 0, "edges_blocked": 0, "neighbours": 0}
    last = {}                                              # host results of the latest cycle (--dump-outputs)

    def cycle(i, timed):
        j = appear[i]
        t = [time.perf_counter()]
        act[j] = 1
        ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)            # the obstacle is sensed: the list changes
        t.append(time.perf_counter())
        ids = ctx.obstacle_sweep_polygon(j, rr, delta, r_min=r_min, cap=1 << 16)
        n_c = ctx.stats().last_sweep_candidates
        t.append(time.perf_counter())
        if len(ids):
            ctx.graph_edges_block(ids)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        lmc, _, _ = ctx.graph_cost_update(root, want_parent=False)
        last.update(blocked_edges=ids, lmc=lmc)
        t.append(time.perf_counter())
        n_now = N + i * B
        ri = synth.ball_radius(n_now, 4, gamma=100.0, delta=10.0)
        ctx.extend_candidates_dubins_dev(d_q[i % RING].data_ptr(), B, ri, rr, r_min, d_off.data_ptr(), d_idx.data_ptr(),
                                         d_key.data_ptr(), d_co.data_ptr(), d_ci.data_ptr(), None, None, d_ho.data_ptr(),
                                         d_hi.data_ptr(), cap, d_need.data_ptr() + 8 * i, d_ni.data_ptr(), d_nd.data_ptr(),
                                         d_un.data_ptr())
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        ctx.nodes_append_dev(d_q[i % RING].data_ptr(), B)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        if timed:
            for k, name in enumerate(phase):
                phase[name] += t[k + 1] - t[k]
            counts["sweep_candidates"] += int(n_c)
            counts["edges_blocked"] += len(ids)

    for i in range(warm):
        cycle(i, False)
    fence()
    k_w = d_need[:warm].tolist()
    if max(k_w) > cap:
        raise SystemExit(f"candidate capacity too small: {max(k_w)} > {cap}")
    t0 = time.perf_counter()
    for i in range(warm, warm + steps):
        cycle(i, True)
    fence()
    dt = time.perf_counter() - t0
    ks = [int(v) for v in d_need[warm:warm + steps].tolist()]
    if max(ks) > cap:
        raise SystemExit(f"candidate capacity too small in a timed cycle: {max(ks)} > {cap}")
    counts["neighbours"] = sum(ks)
    units = counts["sweep_candidates"] + 2 * sum(ks)           # directed Dubins edges put through explicitEdgeCheck
    if args.dump_outputs and rank == 0:
        k = ks[-1]
        dump_outputs(args.dump_outputs, {"blocked_edges": last["blocked_edges"], "lmc": last["lmc"], "offsets": d_off,
                                         "idx": d_idx[:k], "key": d_key[:k], "cost_out": d_co[:k], "cost_in": d_ci[:k],
                                         "hit_out": d_ho[:k], "hit_in": d_hi[:k], "nearest_idx": d_ni, "nearest_dist": d_nd,
                                         "sample_unsafe": d_un})
    if args.full:
        # per-family device time of the last cycle's preamble
        ctx.profile(2)
        r_last = synth.ball_radius(N + (warm + steps) * B, 4, gamma=100.0, delta=10.0)
        ctx.extend_candidates_dubins_dev(d_q[0].data_ptr(), B, r_last, rr, r_min, d_off.data_ptr(), d_idx.data_ptr(),
                                         d_key.data_ptr(), d_co.data_ptr(), d_ci.data_ptr(), None, None, d_ho.data_ptr(),
                                         d_hi.data_ptr(), cap, d_need.data_ptr() + 8 * (steps + warm), d_ni.data_ptr(),
                                         d_nd.data_ptr(), d_un.data_ptr())
        fence()
        st = ctx.stats()
        ctx.profile(0)
        if int(d_need[steps + warm].item()) > cap:
            raise SystemExit("candidate capacity too small in the profiled pass")
    e_sum, t_max = parallel.reduce_throughput(units, dt, device=dev)
    if rank == 0:
        rk = make_run_key(args)
        out = {
            "metric": METRIC, "value": e_sum / t_max, "unit": "edges/s", "n_gpus": world, "steps": steps, "warmup": warm,
            "ms_per_step": 1e3 * t_max / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": cfg.name + " -- one replanning cycle per step", "n_nodes": N, "n_obstacles": M,
                       "moving_obstacles": len(moving), "batch_per_gpu": B, "radius": r, "edge": "DubinsEdge with time",
                       "min_turning_radius": r_min, "delta": delta,
                       "edge_mirror": {"directed_edges": int(len(es)), "r_graph": r_graph,
                                       "out_edges_per_node": len(es) / N,
                                       "note": "both directed edges of every pair of nodes within r_graph; the live RRT^X graph "
                                               "at this ball radius would hold ~2 400 out-edges per node"},
                       "cycle": "obstacle appears -> rrtx_obstacle_sweep_polygon -> rrtx_graph_edges_block -> "
                                "rrtx_graph_cost_update -> rrtx_extend_candidates_dubins_dev (fresh batch, r of the current n) "
                                "-> rrtx_nodes_append_dev",
                       "sharding": "replicas only: every rank its own planner (tree, obstacle list, edge mirror)"},
            "phase_ms": {k: 1e3 * v / steps for k, v in phase.items()},
            "per_cycle": {k: v / steps for k, v in counts.items()},
            "initial_solve": {"root": root, "passes": int(passes0), "reachable_nodes": int(np.isfinite(lmc0).sum()),
                              "edges_forward_in_reverse_time": n_valid},
            "run_key": rk, "hip_runtime": _capi.hip_runtime(), "lib_sha16": lib_sha16(), "source_sha16": source_sha16(),
        }
        if args.full:
            d_kernel = "dubins_check_rec_kernel<true>"
            tj = load_pmc(d_kernel, rk)
            chk_launches = int(st.launches_dubins)
            if tj:
                tj = dict(tj)
                for kk in ("SQ_INSTS_VALU_per_launch", "SQ_INSTS_SALU_per_launch", "traffic_bytes_per_launch"):
                    if tj.get(kk) is not None:
                        tj[kk] = tj[kk] * chk_launches
            out["kernel_ms"] = {"nn_scan": st.ms_nn_scan / max(st.launches_nn_scan, 1), "nn_finish": st.ms_nn_finish,
                                "dubins_check": st.ms_dubins, "dubins_steer": st.ms_dubins_steer,
                                "dubins_check_launches": chk_launches, "points": st.ms_points}
            out["roofline"] = issue_roofline(d_kernel, tj, st.ms_dubins,
                                             "; kernel_ms and the instruction counts are the SUM over the check kernel's launches "
                                             "of one preamble (both directions, every chunk of 2 M edges)")
        if world == 1 and args.full and not args.no_cpu_baseline:
            act0 = act.copy()
            out["cpu_baseline"] = cpu_baseline_c5(pts, es, ee, polys, kinds, paths, act0, appear[warm], Qs[warm % RING], r,
                                                  r_min, rr, delta)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


def spawn_ranks(n: int) -> int:
    """One process per GPU through torch.distributed.run on 127.0.0.1 (the launcher the driver itself uses); the
    ranks' output is passed through and their exit code is ours."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC only on this host driver (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"bench.py: --gpus {n} without a launcher, starting {n} ranks: {' '.join(cmd[1:8])} ...", file=sys.stderr, flush=True)
    # stdout carries ONE JSON line: whatever else the ranks' libraries print there (gloo's connection banner ...) goes
    # to stderr, the bench line is printed last
    pr = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in pr.stdout:
        t = ln.strip()
        if t.startswith("{") and t.endswith("}"):
            try:
                json.loads(t)
                line = t
                continue
            except ValueError:
                pass
        sys.stderr.write(ln)
    rc = pr.wait()
    if rc != 0:
        print(f"bench.py: the {n}-rank run failed with exit code {rc}", file=sys.stderr, flush=True)
    elif line is None:
        print(f"bench.py: the {n}-rank run printed no bench line", file=sys.stderr, flush=True)
        rc = 1
    else:
        print(line, flush=True)
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--exchange-every", type=int, default=4,
                    help="multi-GPU: the collision bitmasks of this many steps travel in one all-reduce")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="only the timed line (no steady-state, polygon, host-path passes)")
    ap.add_argument("--nn-filter", type=int, default=1, help="1: fp32 prefilter + exact fp64 confirm (default); 0: exact scan")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for rehearsal)")
    ap.add_argument("--share-device", action="store_true", help="rehearsal: all ranks on cuda:0")
    ap.add_argument("--scan-blocks", type=int, default=0, help="tuning: target workgroups of the range scan")
    ap.add_argument("--scan-items", type=int, default=0, help="tuning: target (tile, segment) work items")
    ap.add_argument("--tile-q", type=int, default=0, help="tuning: query copies per workgroup tile")
    ap.add_argument("--nn-cull", type=int, default=1, help="slab culling of the range scan: 0 off, 1 auto, 2 always")
    ap.add_argument("--tune", type=int, default=0, help="RRTX_OPT_TUNE bit mask (kernel variants under measurement)")
    ap.add_argument("--agents", type=int, default=0, help="side measurement: k independent planners sharing the GPU (0/1: off)")
    ap.add_argument("--batch", type=int, default=0, help="samples per step (0: the config's; e.g. 131072 for a strong-scaling "
                                                         "line that is not launch bound)")
    ap.add_argument("--obstacles", default="spheres", choices=["spheres", "polygons"],
                    help="obstacle list of the timed line (spheres: the reference's 3-D planner; polygons: north_star's wording)")
    ap.add_argument("--shard", default="edges", choices=["edges", "obstacles"],
                    help="multi-GPU: what the ranks split -- the sample / candidate-edge batch (default), or the obstacle list "
                         "(every rank checks all edges against its obstacles, flags OR-reduced with all_reduce(MAX))")
    ap.add_argument("--grid", default="", help="multi-GPU: ExO = E edge shards x O obstacle shards (E * O = --gpus)")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements: per-kernel times and rooflines, CPU baselines, the other scaling mode, "
                         "large-batch, steady-state, host-pointer and polygon passes (a plain run times the headline step only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the arrays the last timed step computed as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    # `python bench.py --gpus N` without a launcher: start the N ranks ourselves.  This happens BEFORE anything touches
    # the GPU (no torch import yet), as a child process -- a process that has initialised HIP must never be replaced.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)

    import torch
    import torch.distributed as dist

    from rrtqx_3d_amd import _capi, parallel, synth
    from rrtqx_3d_amd.context import Context

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: a line that says n_gpus = {world} would not be the run "
                         f"that was asked for")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if args.share_device:            # rehearsal of the N>1 code path on a one-GPU box (with --backend gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)      # RCCL over xGMI
        else:
            dist.init_process_group(args.backend)

    if args.config == "C3":
        return bench_c3(args, torch, dist, dev, rank, world)
    if args.config == "C5":
        return bench_c5(args, torch, dist, dev, rank, world)
    cfg = synth.CONFIGS[args.config]
    assert cfg.dim == 3, "the bench line is the SimpleEdge path (--config C3 for the Dubins preamble)"
    N, M, B = cfg.n_nodes, cfg.n_obstacles, (args.batch or cfg.batch)
    r = synth.ball_radius(N, 3)
    pts = synth.nodes(N, 3)
    sph = synth.spheres(M)
    # ---- the rank grid: E edge (sample) shards x O obstacle shards, rank = e * O + o (parallel.py) ----
    E, O = world, 1
    if args.grid:
        try:
            E, O = (int(v) for v in args.grid.lower().split("x"))
        except ValueError:
            raise SystemExit(f"--grid {args.grid}: expected ExO, e.g. 4x2")
        if E * O != world:
            raise SystemExit(f"--grid {args.grid} needs {E * O} ranks, WORLD_SIZE = {world}")
    elif args.shard == "obstacles":
        E, O = 1, world
    e_idx, o_idx = parallel.grid_of(rank, world, E, O)
    obs_group = parallel.obstacle_groups(world, E, O, rank)
    use_polys = args.obstacles == "polygons"
    o_lo, o_hi = parallel.shard_range(M, o_idx, O)           # this rank's list positions
    extras_on = args.full and not args.no_extras
    steady_steps = 0 if (not extras_on or use_polys or O > 1 or args.batch) else args.steps
    ctx = Context(3, device=local_rank, node_capacity=N)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)          # kernels, events and torch share one stream
    if use_polys:
        polys_all = synth.polygons(M)
        ctx.polygons_set(polys_all[o_lo:o_hi])
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
    else:
        ctx.spheres_set(sph[o_lo:o_hi])
    ctx.set_option(_capi.RRTX_OPT_NN_FILTER, args.nn_filter)
    if args.scan_blocks:
        ctx.set_option(_capi.RRTX_OPT_SCAN_BLOCKS, args.scan_blocks)
    if args.scan_items:
        ctx.set_option(_capi.RRTX_OPT_SCAN_ITEMS, args.scan_items)
    if args.tile_q:
        ctx.set_option(_capi.RRTX_OPT_SCAN_TILE_Q, args.tile_q)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, args.nn_cull)
    if args.tune:
        ctx.set_option(_capi.RRTX_OPT_TUNE, args.tune)

    # ---- inputs resident in HBM before the timed region -----------------------
    d_pts = torch.from_numpy(pts).to(dev)
    ctx.nodes_append_dev(d_pts.data_ptr(), N)
    cap = 96 * B                                 # expected sum(k) ~ 26 B; generous head room

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def make_mode(mode, batch=None):
        """weak: every EDGE shard its own ring of B-sample batches; strong: a ring of GLOBAL batches (same seed on
        every rank), of which edge shard e takes its shard_range.  The O ranks of an obstacle group hold the same
        samples (each checks them against its own obstacles)."""
        Bm = batch or B
        capm = 96 * Bm
        if mode == "weak" or E == 1:
            lo, hi = 0, Bm
            batches = [synth.queries(Bm, 3, seed=synth.SEED + 1 + 1000 * e_idx + 17 * j) for j in range(RING)]
        else:
            lo, hi = parallel.shard_range(Bm, e_idx, E)
            batches = [synth.queries(Bm, 3, seed=synth.SEED + 1 + 17 * j)[lo:hi] for j in range(RING)]
        nb = hi - lo
        d_q = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in batches]
        buf = Buffers(torch, dev, max(nb, 1), capm)
        d_need = torch.zeros(RING, dtype=torch.int64, device=dev)
        return {"mode": mode, "nb": nb, "host_q": batches, "q": d_q, "buf": buf, "need": d_need, "B": Bm}

    def compute(m, j):
        b = m["buf"]
        ctx.extend_candidates_dev(m["q"][j].data_ptr(), m["nb"], r, ROBOT_RADIUS, b.off.data_ptr(), b.idx.data_ptr(),
                                  b.cost.data_ptr(), b.hout.data_ptr(), b.hin.data_ptr(), b.cap,
                                  m["need"].data_ptr() + 8 * j, b.nidx.data_ptr(), b.ndist.data_ptr(),
                                  b.unsafe.data_ptr())

    def run_mode(m, steps, warmup, profile):
        """times `steps` steps of mode m; returns (directed edges of this rank over the steps, seconds, stats, ...)"""
        # sizing pass (part of the warm-up): candidate entries of every batch of the ring
        for j in range(RING):
            compute(m, j)
        fence()
        k_ring = [int(v) for v in m["need"].tolist()]
        if max(k_ring) > m["buf"].cap:
            raise SystemExit(f"candidate capacity too small: {max(k_ring)} > {m['buf'].cap}")
        # exchange buffers sized for the largest shard: 2 bits (out, in) per candidate entry and rank
        k_max = max(k_ring)
        if world > 1:
            t = torch.tensor([k_max], dtype=torch.int64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            k_max = int(t.item())
        bit_cap = (k_max + 4095) // 4096 * 4096
        wpr = parallel.words_for(bit_cap)
        K = max(1, args.exchange_every)
        # edge shards only: every rank publishes -> one all-gather, buffer [ranks, steps, words] (half the ring traffic of
        # the all-reduce over disjoint slices, which stays for E x O grids where one rank per obstacle group publishes)
        gathered = O == 1
        d_bits = [torch.zeros((E, K, wpr) if gathered else (K, E, wpr), dtype=torch.int64, device=dev) for _ in range(2)]
        pending = [None, None]
        if O > 1:
            # obstacle shards: the flag arrays are re-allocated at exactly the exchanged size, so that hit_out | hit_in |
            # sample flags of a step are ONE contiguous message of 2 * bit_cap + nb bytes for the OR-reduce
            m["buf"] = Buffers(torch, dev, max(m["nb"], 1), bit_cap)
            for j in range(RING):
                compute(m, j)
            fence()
        b = m["buf"]
        own = e_idx if o_idx == 0 else None          # one rank of every obstacle group publishes the group's bitmask

        def step(i, last=False):
            j = i % RING
            compute(m, j)
            if O > 1:
                # north_star's obstacle-set shard: every rank of the group has checked the same edges against ITS
                # obstacles; OR over the group = all_reduce(MAX) of the flag bytes (RCCL has no bitwise OR)
                parallel.reduce_obstacle_shards(b.flags, group=obs_group)
            if world > 1:
                # per-edge collision bitmask exchange: each rank packs its slice of the step, and the slices of K
                # steps travel in ONE RCCL all-reduce (disjoint slices: SUM == OR; xGMI rings are latency bound at
                # these sizes).  Double-buffered and asynchronous: the exchange of a group of steps runs on RCCL's
                # stream while the next group computes.
                s, slot = (i // K) & 1, i % K
                if slot == 0 and pending[s] is not None:
                    pending[s].wait()
                    pending[s] = None
                if own is not None:
                    ctx.pack_hits_dev(b.hout.data_ptr(), b.hin.data_ptr(), b.off.data_ptr() + 8 * m["nb"], bit_cap,
                                      d_bits[s].data_ptr() + 8 * ((e_idx * K + slot) if gathered else (slot * E + e_idx)) * wpr)
                if slot == K - 1 or last:
                    pending[s] = exchange(d_bits[s], async_op=True)

        def exchange(bits, async_op=False):
            if gathered:
                return parallel.exchange_hit_bitmasks_gathered(bits, e_idx, async_op=async_op)
            return parallel.exchange_hit_bitmasks_grouped(bits, own, async_op=async_op)

        def drain():
            for s in range(2):
                if pending[s] is not None:
                    pending[s].wait()
                    pending[s] = None

        for i in range(warmup):
            step(i, last=(i == warmup - 1))
        drain()
        if world > 1:
            # both exchange buffers have been through the collective once before the clock starts (first use of a
            # buffer pays registration / staging set-up in the backend)
            for s in range(2):
                exchange(d_bits[s])
        fence()
        # (every 10th step of a default run: an instrumented step costs ~10 us more, every 4th step was 2.5 us of a
        #  54 us step -- tools/graph_probe.py times the same calls without events at 0.0516 ms)
        sample_every = 10 if steps >= 20 else (4 if steps >= 8 else 1)
        if profile:
            # HIP events around the dominant kernel only, and only on every n-th step: two event records
            # drain the pipeline for ~10 us
            ctx.set_option(_capi.RRTX_OPT_PROFILE_EVERY, sample_every)
            ctx.profile(1)
        fence()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i, last=(i == steps - 1))
        drain()
        fence()
        dt = time.perf_counter() - t0
        st = ctx.stats() if profile else None
        if profile:
            ctx.set_option(_capi.RRTX_OPT_PROFILE_EVERY, 1)
            ctx.profile(0)
        # units: directed edges of this EDGE shard; the other ranks of its obstacle group checked the same edges
        edges = sum(2 * k_ring[i % RING] for i in range(steps)) if o_idx == 0 else 0
        return edges, dt, st, k_ring, sample_every

    # a plain run: the headline mode alone, no events in its timed loop; --full: in-loop kernel events and the other mode
    modes = [args.scaling] + ([("strong" if args.scaling == "weak" else "weak")] if E > 1 and args.full else [])
    results = {}
    for mode in modes:
        m = make_mode(mode)
        edges, dt, st, k_ring, sample_every = run_mode(m, args.steps, args.warmup, profile=args.full and mode == modes[0])
        e_sum, t_max = parallel.reduce_throughput(edges, dt, device=dev)
        results[mode] = {"m": m, "edges": edges, "dt": dt, "st": st, "k_ring": k_ring, "e_sum": e_sum, "t_max": t_max,
                         "sample_every": sample_every}
        if mode == modes[0] and args.dump_outputs and rank == 0:
            # the buffers still hold the last timed step (batch (steps - 1) % RING) of this rank
            b, nb, k = m["buf"], m["nb"], k_ring[(args.steps - 1) % RING]
            dump_outputs(args.dump_outputs, {"offsets": b.off[:nb + 1], "idx": b.idx[:k], "cost": b.cost[:k],
                                             "hit_out": b.hout[:k], "hit_in": b.hin[:k], "nearest_idx": b.nidx[:nb],
                                             "nearest_dist": b.ndist[:nb], "sample_unsafe": b.unsafe[:nb]})
    large = None
    if extras_on and not args.batch:
        # the same step at a batch that is several grid waves per kernel (B = 131072): strong-sharded over the edge
        # shards when there are any -- at B = 16384 a step is four launch-bound kernels and splitting it removes
        # workgroups, not chain length; this is the line where splitting the batch can pay
        lb = make_mode("strong" if E > 1 else "weak", batch=131072)
        l_steps = max(5, args.steps // 2)
        l_edges, l_dt, _, l_ring, _ = run_mode(lb, l_steps, 2, profile=False)
        le, lt = parallel.reduce_throughput(l_edges, l_dt, device=dev)
        large = {"global_batch": 131072, "batch_per_edge_shard": lb["nb"], "scaling": "strong" if E > 1 else "single",
                 "value": le / lt, "ms_per_step": 1e3 * lt / l_steps, "steps": l_steps,
                 "directed_edges_per_step": 2 * sum(l_ring) / len(l_ring) * (E if E > 1 else 1)}
        del lb
    main_r = results[modes[0]]
    m = main_r["m"]
    st = main_r["st"]
    k_ring = main_r["k_ring"]
    k_mean = sum(k_ring) / len(k_ring)

    extras = {}
    if extras_on:
        # per-family device time in a short pass of its own (an event record between two kernels costs
        # ~10 us of pipeline drain, which must not sit inside the timed region)
        ctx.profile(2)
        for i in range(5):
            compute(m, i % RING)
        fence()
        st_all = ctx.stats()
        ctx.profile(0)
        extras["kernel_ms_all"] = {"nn_pack_place_finish": st_all.ms_nn_finish / 5,
                                   "nn_scan_separate_pass": st_all.ms_nn_scan / max(st_all.launches_nn_scan, 1)}
        if use_polys:
            extras["kernel_ms_all"].update({"edges_polygons": st_all.ms_edges / 5, "points_polygons": st_all.ms_points / 5})
        # the brute-force form of the search (every tile of 64 copies streams every node, north_star's
        # kernel) measured beside the default culled form: a short pass with culling switched off
        if args.nn_filter and args.nn_cull and st.last_scan_units > 0:
            ctx.set_option(_capi.RRTX_OPT_NN_CULL, 0)
            compute(m, 0)
            fence()
            ctx.profile(1)
            for i in range(5):
                compute(m, 0)
            fence()
            st_bf = ctx.stats()
            extras["bf"] = {"scan_ms": st_bf.ms_nn_scan / max(st_bf.launches_nn_scan, 1), "tile_q": int(st_bf.last_tile_q)}
            ctx.set_option(_capi.RRTX_OPT_NN_CULL, args.nn_cull)
            ctx.profile(0)
            compute(m, 0)
            fence()

    # ---- steady state: the tree grows by the batch after every step (kdInsert of every sample, R/DRRT_Q.jl:2575)
    #      and the ball shrinks with it (R/rrtqx.jl:382), so index tails and rebuilds are inside the timing ----
    steady = None
    if steady_steps > 0 and modes[0] == "weak":
        d_need_s = torch.zeros(steady_steps + 1, dtype=torch.int64, device=dev)
        sctx = Context(3, device=local_rank, node_capacity=N + (steady_steps + 2) * B)
        sctx.set_stream(stream.cuda_stream)
        sctx.spheres_set(sph)
        sctx.nodes_append_dev(d_pts.data_ptr(), N)
        bufs = m["buf"]

        def sstep(i, slot):
            n_now = N + i * B
            rr = synth.ball_radius(n_now, 3)
            sctx.extend_candidates_dev(m["q"][i % RING].data_ptr(), B, rr, ROBOT_RADIUS, bufs.off.data_ptr(),
                                       bufs.idx.data_ptr(), bufs.cost.data_ptr(), bufs.hout.data_ptr(), bufs.hin.data_ptr(),
                                       cap, d_need_s.data_ptr() + 8 * slot, bufs.nidx.data_ptr(), bufs.ndist.data_ptr(),
                                       bufs.unsafe.data_ptr())
            sctx.nodes_append_dev(m["q"][i % RING].data_ptr(), B)

        sstep(0, steady_steps)       # warm-up (buffers, index build); the tree keeps the batch
        fence()
        t0 = time.perf_counter()
        for i in range(steady_steps):
            sstep(i + 1, i)
        fence()
        dts = time.perf_counter() - t0
        ks = d_need_s[:steady_steps].tolist()
        e_s, t_s = parallel.reduce_throughput(int(2 * sum(ks)), dts, device=dev)
        steady = {"value_steady": e_s / t_s, "ms_per_step": 1e3 * t_s / steady_steps, "steps": steady_steps,
                  "n_nodes_start": N + B, "n_nodes_end": N + (steady_steps + 1) * B,
                  "neighbors_per_step_first_last": [int(ks[0]), int(ks[-1])],
                  "note": "every step: fused extend() preamble on a fresh batch with r = min(delta, gamma (ln(1+n)/n)^(1/3)) "
                          "for the current n, then rrtx_nodes_append_dev of the whole batch (every sample inserted: upper "
                          "bound on the reference's accepted samples); index tail growth and slab-index rebuilds are inside "
                          "the timed loop"}
        sctx.close()

    if rank == 0:
        e_sum, t_max = main_r["e_sum"], main_r["t_max"]
        nb = m["nb"]
        ms_step = 1e3 * t_max / args.steps
        rk = make_run_key(args)
        out = {
            "metric": METRIC,
            "value": e_sum / t_max,
            "unit": "edges/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": modes[0],
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": cfg.name, "n_nodes": N, "n_obstacles": M,
                       "batch_per_gpu": nb, "global_batch": nb * E if modes[0] == "weak" else B,
                       "obstacle_list": "polygons" if use_polys else "spheres",
                       "grid": {"edge_shards": E, "obstacle_shards": O, "obstacles_per_rank": o_hi - o_lo},
                       "radius": r, "edge": "SimpleEdge", "directed_edges_per_step_per_gpu": 2 * k_mean,
                       "neighbors_per_step_per_gpu": k_mean, "fresh_batch_every_step": True, "batch_ring": RING,
                       "sharding": ("samples+edges sharded, nodes/obstacles replicated" if O == 1 else
                                    "%d edge shard(s) x %d obstacle shards: every rank of an obstacle group checks the group's "
                                    "edges against its %d obstacles; nodes replicated" % (E, O, o_hi - o_lo)),
                       "collective": (None if world == 1 else
                                      (("all_reduce(MAX) of the uint8 edge / sample flags inside every obstacle group each step "
                                        "(OR over obstacle shards), then " if O > 1 else "") +
                                       ("one RCCL all-gather" if O == 1 else "one RCCL all-reduce (disjoint slices)") +
                                       " of the per-edge collision bitmasks of %d steps, asynchronous, double-buffered"
                                       % max(1, args.exchange_every)))},
            "nn_queries_per_s": (nb * E if modes[0] == "weak" else B) * args.steps / t_max,
            "launches_per_step": 4,
            "run_key": rk,
            "hip_runtime": _capi.hip_runtime(),
            "lib_sha16": lib_sha16(),
            "source_sha16": source_sha16(),
        }
        if args.full:
            scan_ms = st.ms_nn_scan / max(st.launches_nn_scan, 1)
            tile_q = int(st.last_tile_q)   # query copies sharing one streamed pass of the node arrays
            n_tiles = (nb + tile_q - 1) // tile_q
            units = int(st.last_scan_units)  # slab-culled scan: (tile, 512-node chunk) pairs actually streamed (last call)
            k_last = k_ring[(args.steps - 1) % RING]
            node_visits = units * 512 if units > 0 else n_tiles * N
            # SURVEY 8(d) contract figure: node passes x 24 B (fp64 x, y, z of every node visit) + queries + hit records
            bytes_alg = node_visits * 24 + nb * 32 + k_last * 16
            # what the kernel really requests: the fp32 screen record of a node is 16 B (x, y, z, |p|^2); each entry the
            # screen leaves over re-reads the fp64 rows of its lane's 8 nodes (3 x 64 B); 16-B hit records out
            culled = units > 0
            kernel = (("nn_tile_kernel<3, false>" if use_polys else "nn_tile_kernel<3, true>") if culled
                      else "nn_scan_f32_kernel<3> + nn_confirm_kernel<3>") if args.nn_filter else "nn_scan_kernel<3>"
            bytes_req = node_visits * 16 + nb * 48 + k_last * (192 + 16 + 8)
            # the in-loop figure comes from few launches (every 10th step carries events); the separate pass times EVERY launch
            scan_ms_loop = scan_ms
            sep = extras.get("kernel_ms_all", {}).get("nn_scan_separate_pass")
            if sep:
                scan_ms = sep
            alg_gbs = bytes_alg / (scan_ms * 1e-3) / 1e9
            traffic, traffic_src, frac_traffic, hbm_gbs, issue = None, None, None, None, None
            # counters cannot be read inside this process; the committed PMC passes count only when they were taken on
            # these kernel sources AND this run key (configuration, obstacle list, batch, tuning options)
            tj = load_pmc(kernel, rk) if world == 1 else None
            if tj and tj.get("traffic_bytes_per_launch"):
                traffic = tj["traffic_bytes_per_launch"]
                traffic_src = f"{tj['file']} (rocprofv3 PMC passes, sources {tj['source_sha16']}, lib match {tj['lib_match']})"
                hbm_gbs = traffic / (scan_ms * 1e-3) / 1e9
                frac_traffic = hbm_gbs / HBM_PEAK_GBS
            issue = issue_block(tj, scan_ms)
            roof_bf = None
            bf = extras.get("bf")
            if bf:
                nt = (nb + bf["tile_q"] - 1) // bf["tile_q"]
                by = nt * N * 24 + nb * 32 + k_ring[0] * 16
                ach = by / (bf["scan_ms"] * 1e-3) / 1e9
                roof_bf = {"kernel": "nn_scan_f32_kernel<3> + nn_confirm_kernel<3> (RRTX_OPT_NN_CULL=0)", "bound": "hbm",
                           "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                           "algorithmic_bytes_per_launch": by, "tile_q": bf["tile_q"], "ms": bf["scan_ms"],
                           "pairs_per_s": nb * N / (bf["scan_ms"] * 1e-3)}
            out["kernel_ms"] = {"nn_scan": scan_ms, **extras.get("kernel_ms_all", {})}
            out["roofline"] = {
                "kernel": kernel, "bound": "hbm", "achieved": alg_gbs, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": alg_gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_unit": "bytes/launch",
                "traffic_source": traffic_src,
                "algorithmic_GBps": alg_gbs, "algorithmic_bytes_per_launch": bytes_alg,
                "requested_bytes_per_launch": bytes_req, "frac_requested": bytes_req / (scan_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "hbm_GBps": hbm_gbs, "frac_traffic": frac_traffic, "issue": issue,
                "tile_q": tile_q, "kernel_ms": scan_ms, "kernel_ms_in_loop": scan_ms_loop,
                "timed_launches_in_loop": int(st.launches_nn_scan),
                "timing": (f"kernel_ms: HIP events around every launch of a separate 5-step pass; kernel_ms_in_loop: around "
                           f"every {main_r['sample_every']}th launch inside the timed region") if sep else
                          f"HIP events around every {main_r['sample_every']}th launch inside the timed region",
                "culled_units": units, "node_visits_per_launch": node_visits,
                "node_visits_unculled": n_tiles * N,
                "pairs_per_s": nb * N / (scan_ms * 1e-3),
                "valu_fp64_frac": (nb * N * 9 / (scan_ms * 1e-3) / 1e12 / FP64_VALU_PEAK_TOPS) if not args.nn_filter else None,
                "note": ("`achieved` / `frac` are the SURVEY 8(d) CONTRACT figure (node visits x 24 B per visit at T_q = tile_q, "
                         "/ kernel time; a visit = one node screened against the tile's copies, counted in groups of eight) -- "
                         "algorithmic bytes, not bytes moved from HBM.  The figure counts work the kernel does NOT avoid: since "
                         "the tiles are also cut by the third coordinate the kernel visits 3.5x fewer nodes than the build of "
                         "the middle of round 2 (`culled_units` 11 425 -> ~3 250) and is 1.35x faster, so its contract "
                         "fraction fell from 0.44 to ~0.19 while the edges/s rose; the brute-force form of the search "
                         "(`roofline_bruteforce`, north_star's kernel) is the one the contract figure describes.  The kernel "
                         "streams the 16-B fp32 screen record of a node (`frac_requested`), its working set is L2-resident, "
                         "the counters (`traffic`, `frac_traffic`) are the HBM-side truth and `issue` says what bounds it "
                         "(instruction issue + the dependency chain of one workgroup), see DESIGN.md 4.1.  The same kernel "
                         "also decides both collision flags of every neighbour (fused extend path).") if culled else
                        "VALU-issue bound, node arrays are L2-resident; see DESIGN.md",
            }
            out["roofline_bruteforce"] = roof_bf
        if len(modes) > 1:
            o = results[modes[1]]
            out["other_scaling"] = {"scaling": modes[1], "value": o["e_sum"] / o["t_max"],
                                    "ms_per_step": 1e3 * o["t_max"] / args.steps, "batch_per_gpu": o["m"]["nb"],
                                    "note": ("strong: ONE global batch of B samples per step split with parallel.shard_range; "
                                             "at B = 16384 a step is four dependent launch-bound kernels, so the per-step "
                                             "floor bounds the speed-up") if modes[1] == "strong" else
                                            "weak: every rank its own B-sample batches"}
        if use_polys and "edges_polygons" in extras.get("kernel_ms_all", {}):
            out["roofline_polygon_edges"] = issue_roofline("edges_polygons_kernel", load_pmc("edges_polygons_kernel", rk),
                                                           extras["kernel_ms_all"]["edges_polygons"])
        if large:
            out["large_batch"] = large
        if steady:
            out["steady_state"] = steady
            out["value_steady"] = steady["value_steady"]
        if world == 1 and extras_on and not use_polys:
            # the same step through the host-pointer entry point (what a ccall from Julia pays):
            # H2D of the samples, kernels, D2H of lists/costs/flags.  Reported, never `value`.
            ctx.set_stream(None)
            Q0 = m["host_q"][0]
            hb = {}
            for label, reg in (("pageable_arrays", False), ("registered_arrays", True)):
                ob = ctx.extend_out_buffers(nb, cap, register=reg)          # allocated once, as a Julia host would
                for a in ob.values():
                    a.fill(0)                                                # (touch the pages before the clock starts)
                ctx.extend_candidates(Q0, r, ROBOT_RADIUS, out=ob)
                t1 = time.perf_counter()
                for _ in range(10):
                    ctx.extend_candidates(Q0, r, ROBOT_RADIUS, out=ob)
                dth = (time.perf_counter() - t1) / 10
                hb[label] = {"ms_per_step": dth * 1e3, "edges_per_s": 2 * k_ring[0] / dth}
                if reg:
                    for a in ob.values():
                        ctx.host_unregister(a)
            out["host_buffer_path"] = {**hb["pageable_arrays"], "registered_arrays": hb["registered_arrays"],
                                       "bytes_out_per_step": int(k_ring[0] * 14 + nb * 21 + 8),
                                       "note": "PCIe-inclusive: rrtx_extend_candidates with host numpy arrays in and out that the "
                                               "caller keeps across calls; results travel through the context's pinned staging "
                                               "arena + one memcpy per array (ms_per_step), or by direct DMA into arrays the "
                                               "caller registered with rrtx_host_register (registered_arrays)"}
            # BASELINE.json's config text says "polygon obstacles": the reference's 3-D planner checks
            # spheres (explicitEdgeCheck3D) and `value` above is that; this is the same step against 256
            # random polygons in the (x, y) projection (explicitEdgeCheck2D), device-resident, reported only.
            ctx.set_stream(stream.cuda_stream)
            ctx.polygons_set(synth.polygons(M))
            ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
            for _ in range(3):
                compute(m, 0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(20):
                compute(m, i % RING)
            torch.cuda.synchronize()
            dtp = (time.perf_counter() - t1) / 20
            ctx.profile(2)
            for i in range(5):
                compute(m, 0)
            torch.cuda.synchronize()
            stp = ctx.stats()
            ctx.profile(0)
            b = m["buf"]
            kt = k_ring[0]
            coll = float((b.hout[:kt].sum() + b.hin[:kt].sum()).item()) / (2 * kt)
            edges_ms = stp.ms_edges / 5
            # a directed edge against the polygon list = 32 B of edge + M (24 B centre/radius + P x 16 B): the
            # LOGICAL bytes of the reference's loop.  The kernel never moves them (the table is 22 KB and every wave drops
            # ~244 of 256 obstacles by their boxes), so they are no roofline; what bounds the kernel is instruction issue.
            pbar = 3.5
            by_poly = 2 * kt * 32 + 2 * kt * M * (24 + pbar * 16)
            rf_poly = issue_roofline("edges_polygons_kernel", load_pmc("edges_polygons_kernel", make_run_key(args, obstacles="polygons")),
                                     edges_ms)
            rf_poly["algorithmic_bytes_logical"] = by_poly
            out["polygon_obstacles"] = {
                "edges_per_s": 2 * k_mean / dtp, "ms_per_step": dtp * 1e3, "n_polygons": M, "colliding_fraction": coll,
                "kernel_ms": {"edges_polygons": edges_ms, "points_polygons": stp.ms_points / 5,
                              "nn_scan": stp.ms_nn_scan / max(stp.launches_nn_scan, 1), "nn_finish": stp.ms_nn_finish / 5},
                "roofline": rf_poly,
                "note": "same samples and tree, candidate edges and samples checked against the polygon list"}
            ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 0)
            ctx.set_stream(None)
        if world == 1 and args.agents > 1:
            out["concurrent_agents"] = concurrent_agents(args.agents, torch, dev, pts, sph, r, B, cap, N)
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg, pts, m["host_q"][0], sph, r, polys=polys_all if use_polys else None)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
