"""Every result of the full-size searches and of the SimpleEdge extend() preamble against the batched CPU oracle, bit
for bit: the C4 headline step against its 256 spheres and its 256 polygons through every placement route and every
caller, the stand-alone edge check over all directed edges, k nearest at C4, the C5s / C3 / C5 range searches and a
steady state that grows the C4 tree past an index rebuild.  The oracle's batch forms loop its per-query functions on
up to 16 threads (tests/test_oracle_range_batch.py holds them to those functions); each oracle result is built once
per module."""
import math
import time

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR = 0.5
OLD_ROUTE = 4                                   # RRTX_OPT_TUNE bit: pack -> place -> tile
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")
EDGE_FIELDS = ("hit_out", "hit_in", "first_hit_out", "first_hit_in")
RANGE_FIELDS = ("offsets", "idx", "key")
_CACHE = {}


def _c4(oracle):
    """C4's tree, batch and radius with the oracle's range + nearest result for every sample (shared by the sphere
    and the polygon scene: same points, samples and r)"""
    if "c4" not in _CACHE:
        cfg = synth.CONFIGS["C4"]
        pts, Q, r = synth.nodes(cfg.n_nodes, 3), synth.queries(cfg.batch, 3), synth.ball_radius(cfg.n_nodes, 3)
        t0 = time.perf_counter()
        rng = oracle.range_batch(oracle.TreeSet(3, pts), Q, r, per_sample=40)
        _CACHE["c4"] = dict(pts=pts, Q=Q, r=r, M=cfg.n_obstacles, rng=rng, t=time.perf_counter() - t0)
    return _CACHE["c4"]


def _c4_extend(oracle, kind):
    if kind not in _CACHE:
        s = _c4(oracle)
        obs = oracle.make_spheres(synth.spheres(s["M"])) if kind == "spheres" else oracle.PolygonSet(synth.polygons(s["M"]))
        _CACHE[kind] = oracle.extend_candidates_batch(None, s["Q"], s["r"], s["pts"], obs, RR, rng=s["rng"])
    return _CACHE[kind]


def _every_route_and_caller(oracle, ctx, s, ref, label):
    """the default route (tile-kernel placement), RRTX_OPT_TUNE bit 4 (place pass), RRTX_OPT_NN_CULL = 0 (no culling)
    through the host form; then out= page-locked buffers and extend_candidates_dev on torch buffers"""
    Q, r = s["Q"], s["r"]
    B = len(Q)
    for name, opt, val, place in (("default route", _capi.RRTX_OPT_TUNE, 0, 2),
                                  ("RRTX_OPT_TUNE bit 4", _capi.RRTX_OPT_TUNE, OLD_ROUTE, 1),
                                  ("RRTX_OPT_NN_CULL=0", _capi.RRTX_OPT_NN_CULL, 0, 0)):
        ctx.set_option(opt, val)
        out = ctx.extend_candidates(Q, r, RR)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == place, name
        ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 1)
        oracle.assert_same_results(out, ref, EXTEND_FIELDS, label=f"{label}, {name}: ")
    n = len(ref["idx"])
    bufs = ctx.extend_out_buffers(B, n + 64, register=True)
    try:
        got = ctx.extend_candidates(Q, r, RR, out=bufs)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == 2
        oracle.assert_same_results(got, ref, EXTEND_FIELDS, label=f"{label}, out= page-locked: ")
    finally:
        for a in bufs.values():
            ctx.host_unregister(a)
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(Q).to(dev)
    d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    d_idx = torch.empty(n + 64, dtype=torch.int32, device=dev)
    d_cost = torch.empty(n + 64, dtype=torch.float64, device=dev)
    d_ho = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    d_hi = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    d_need = torch.zeros(1, dtype=torch.int64, device=dev)
    d_ni = torch.empty(B, dtype=torch.int32, device=dev)
    d_nd = torch.empty(B, dtype=torch.float64, device=dev)
    d_un = torch.empty(B, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.extend_candidates_dev(d_q.data_ptr(), B, r, RR, d_off.data_ptr(), d_idx.data_ptr(), d_cost.data_ptr(),
                              d_ho.data_ptr(), d_hi.data_ptr(), n + 64, d_need.data_ptr(), d_ni.data_ptr(),
                              d_nd.data_ptr(), d_un.data_ptr())
    ctx.sync()
    k = int(d_need.item())
    assert k == n
    got = dict(offsets=d_off.cpu().numpy(), idx=d_idx.cpu().numpy()[:k], cost=d_cost.cpu().numpy()[:k],
               hit_out=d_ho.cpu().numpy()[:k], hit_in=d_hi.cpu().numpy()[:k], nearest_idx=d_ni.cpu().numpy(),
               nearest_dist=d_nd.cpu().numpy(), sample_unsafe=d_un.cpu().numpy())
    oracle.assert_same_results(got, ref, EXTEND_FIELDS, label=f"{label}, extend_candidates_dev: ")


def _edges_check_all(oracle, ctx, s, ref, kind, label):
    """the stand-alone edge kernel over all 2n directed edges: hit and first hit of every one"""
    n = len(ref["idx"])
    p0, p1 = synth.candidate_edges(s["Q"], s["pts"], ref["offsets"], ref["idx"])
    hit, first = ctx.edges_check(p0, p1, RR, kind=kind)
    got = dict(offsets=ref["offsets"], hit_out=hit[:n], hit_in=hit[n:], first_hit_out=first[:n], first_hit_in=first[n:])
    oracle.assert_same_results(got, ref, EDGE_FIELDS, label=f"{label}, edges_check: ")
    return 2 * n


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_c4_extend_every_result(oracle, kind):
    s = _c4(oracle)
    ref = _c4_extend(oracle, kind)
    # the oracle's own result is not vacuous: C4's density, both directions, hit rates as measured for each list
    B, n = len(s["Q"]), len(ref["idx"])
    assert B == 16_384 and n > 20 * B and s["rng"]["nearest_idx"].shape == (B,)
    assert np.array_equal(ref["cost"], ref["key"]) and np.array_equal(ref["cost_in"], ref["cost"])
    hits = (ref["hit_out"].mean(), ref["hit_in"].mean())
    if kind == "spheres":
        assert all(0.01 < h < 0.2 for h in hits) and 0 < ref["sample_unsafe"].sum() < 0.1 * B
    else:
        assert all(0.3 < h < 0.8 for h in hits) and 0.1 * B < ref["sample_unsafe"].sum() < 0.8 * B
    assert ((ref["first_hit_out"] >= 0) == (ref["hit_out"] != 0)).all()
    with Context(3, node_capacity=len(s["pts"])) as ctx:
        ctx.nodes_append(s["pts"])
        if kind == "spheres":
            ctx.spheres_set(synth.spheres(s["M"]))
        else:
            ctx.polygons_set(synth.polygons(s["M"]))
            ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        label = f"C4 {kind}"
        _every_route_and_caller(oracle, ctx, s, ref, label)
        edges = _edges_check_all(oracle, ctx, s, ref, 0 if kind == "spheres" else 1, label)
    print(f"\n{label}: {B} samples, {n} entries x 5 routes/callers, {edges} directed edges (edges_check) against the "
          f"oracle; oracle range {s['t']:.1f} s")


def test_knearest_c4_every_query(oracle):
    cfg = synth.CONFIGS["C4"]
    N, B, k = cfg.n_nodes, 2048, 16
    pts, Q = synth.nodes(N, 3), synth.queries(B, 3)
    oi, ok, oc = oracle.knearest_batch(oracle.TreeSet(3, pts), k, Q)
    assert (oc == k).all()
    o = np.lexsort((oi, ok), axis=1)                                   # the device's order: (distance, index)
    oi, ok = np.take_along_axis(oi, o, axis=1), np.take_along_axis(ok, o, axis=1)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        idx, dist, count = ctx.nn_knearest(Q, k)
    rows = dict(offsets=np.arange(B + 1) * k)
    oracle.assert_same_results(dict(rows, nearest_idx=count), dict(rows, nearest_idx=oc), ("nearest_idx",),
                               label="C4 k nearest, count: ")
    oracle.assert_same_results(dict(rows, nearest_idx=idx, nearest_dist=dist),
                               dict(rows, nearest_idx=oi, nearest_dist=ok), ("nearest_idx", "nearest_dist"),
                               label="C4 k nearest: ")
    print(f"\nC4 k nearest: {B} queries x {k} neighbours against the oracle")


def _range_device(ctx, Q, r, cap=None, nearest=False):
    off, idx, dist = ctx.nn_radius(Q, r, cap=cap)
    out = dict(offsets=off, idx=idx, key=dist)
    if nearest:
        out["nearest_idx"], out["nearest_dist"] = ctx.nn_nearest(Q)
    return out


def test_c5s_range_every_sample(oracle):
    cfg = synth.CONFIGS["C5s"]
    N, B = cfg.n_nodes, cfg.batch
    pts, Q, r = synth.nodes(N, 3), synth.queries(B, 3), synth.ball_radius(N, 3)
    ref = oracle.range_batch(oracle.TreeSet(3, pts), Q, r, per_sample=40)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        got = _range_device(ctx, Q, r, nearest=True)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == 2
    assert len(ref["idx"]) > 10 * B
    oracle.assert_same_results(got, ref, RANGE_FIELDS + ("nearest_idx", "nearest_dist"), label="C5s range: ")
    print(f"\nC5s range + nearest: {B} samples, {len(ref['idx'])} entries against the oracle")


def test_c3_range_every_sample(oracle):
    cfg = synth.CONFIGS["C3"]
    N, B = cfg.n_nodes, cfg.batch
    pts, Q = synth.nodes(N, 4), synth.queries(B, 4)
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    ref = oracle.range_batch(oracle.TreeSet(4, pts, wraps=[3], wrap_points=[2.0 * math.pi]), Q, r, per_sample=1500,
                             nearest=False)
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        got = _range_device(ctx, Q, r)
    assert len(ref["idx"]) > 500 * B
    oracle.assert_same_results(got, ref, RANGE_FIELDS, label="C3 range: ")
    print(f"\nC3 range: {B} samples, {len(ref['idx'])} entries against the oracle")


def test_c5_range_slices(oracle):
    """the full C5 batch on the device (wrapped theta, ghosts); samples [0, 2048) -- those whose Dubins preamble
    the Dubins tests check -- and the last 1024 against the oracle"""
    cfg = synth.CONFIGS["C5"]
    N, B = cfg.n_nodes, cfg.batch
    pts, Q = synth.nodes_time(N), synth.nodes_time(B, seed=synth.SEED + 1)
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    sel = np.concatenate([np.arange(2048), np.arange(B - 1024, B)])
    ref = oracle.range_batch(oracle.TreeSet(4, pts, wraps=[3], wrap_points=[2.0 * math.pi]), Q[sel], r,
                             per_sample=2400, nearest=False)
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        got = _range_device(ctx, Q, r, cap=80_000_000)
    assert len(ref["idx"]) > 1000 * len(sel)
    oracle.assert_same_results(oracle.take_samples(got, sel), ref, RANGE_FIELDS, names=sel, label="C5 range: ")
    print(f"\nC5 range: {len(sel)} of {B} samples, {len(ref['idx'])} entries against the oracle")


def test_c4_steady_state(oracle):
    """bench.py's steady pass: every step searches a fresh batch with the radius of the current n, then appends the
    batch to the device and to the oracle's trees.  DESIGN.md section 4.1: at C4's batch the slab index is rebuilt
    after five or six appended runs, so eight steps pass at least one rebuild.  Every step: all samples against the
    unculled device path, a slice of 256 whole tiles (4096 samples) against the oracle."""
    cfg = synth.CONFIGS["C4"]
    N, B, steps, sl = cfg.n_nodes, cfg.batch, 8, 4096
    pts, sph = synth.nodes(N, 3), synth.spheres(cfg.n_obstacles)
    ts = oracle.TreeSet(3, pts)
    osph = oracle.make_spheres(sph)
    allpts = pts
    checked = 0
    with Context(3, node_capacity=N + steps * B) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        for step in range(steps):
            n_now = N + step * B
            r = synth.ball_radius(n_now, 3)
            Q = synth.queries(B, 3, seed=synth.SEED + 100 + step)
            out = ctx.extend_candidates(Q, r, RR)
            assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == 2
            ctx.set_option(_capi.RRTX_OPT_NN_CULL, 0)
            brute = ctx.extend_candidates(Q, r, RR)
            ctx.set_option(_capi.RRTX_OPT_NN_CULL, 1)
            oracle.assert_same_results(out, brute, EXTEND_FIELDS, label=f"steady step {step}, culled vs unculled: ")
            sel = np.arange((step * sl) % B, (step * sl) % B + sl)
            ref = oracle.extend_candidates_batch(ts, Q[sel], r, allpts, osph, RR, per_sample=40)
            oracle.assert_same_results(oracle.take_samples(out, sel), ref, EXTEND_FIELDS, names=sel,
                                       label=f"steady step {step} (n = {n_now}): ")
            if step:
                assert (ref["idx"] >= N).any()                             # the appended batches are found
            checked += len(ref["idx"])
            ctx.nodes_append(Q)
            ts.insert_many(Q)
            allpts = np.concatenate([allpts, Q])
        assert ctx.n_nodes == ts.size == N + steps * B
    print(f"\nC4 steady state: {steps} steps, {steps * B} samples against the unculled path, {steps * sl} samples and "
          f"{checked} entries against the oracle")
