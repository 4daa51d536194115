"""Culled range search without ghosts: the tile kernel places the copies itself from the bucket-slot table the pack
pass fills (three launches), where RRTX_OPT_TUNE bit 4 keeps the place pass (four launches).  Both routes must
return the same arrays, bit for bit, whatever the samples do to the bucket histogram -- and those arrays must be the
CPU oracle's (every sample up to B = 16384; whole tiles spread over the batch at B = 131072, where the unculled path
answers for every sample)."""
import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

OLD_ROUTE = 4          # RRTX_OPT_TUNE bit: pack -> place -> tile
ROBOT_RADIUS = 0.5
TILE = 16              # samples per tile of the range search
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")
RANGE_FIELDS = ("offsets", "idx", "key")
_TREES = {}


def _trees(oracle, pts):
    """the oracle's trees over pts, once per node set of this module"""
    key = (pts.shape, pts.tobytes()[:4096], float(pts.sum()))
    if key not in _TREES:
        _TREES[key] = oracle.TreeSet(pts.shape[1], pts)
    return _TREES[key]


def _spread_tiles(B, samples=16_384):
    """whole tiles spread over the batch, the last tiles among them, at least `samples` samples"""
    nt = B // TILE
    tiles = np.unique(np.concatenate([np.linspace(0, nt - 1, samples // TILE).astype(np.int64), np.arange(nt - 4, nt)]))
    return (tiles[:, None] * TILE + np.arange(TILE)).ravel()


def _vs_oracle(oracle, out, pts, Q, r, obs, sel=None, label="", fields=EXTEND_FIELDS):
    """the route's result against the oracle's extend() preamble on the samples sel (default all); returns the
    oracle's result"""
    sel = np.arange(len(Q)) if sel is None else sel
    ref = oracle.extend_candidates_batch(_trees(oracle, pts), Q[sel], r, pts, obs, ROBOT_RADIUS)
    oracle.assert_same_results(oracle.take_samples(out, sel), ref, fields, names=sel, label=label)
    return ref


def _both_routes(ctx, call):
    outs = []
    for tune, route in ((0, 2), (OLD_ROUTE, 1)):     # RRTX_OPT_LAST_PLACEMENT: 2 tile kernel, 1 place pass
        ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
        outs.append(call())
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == route
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    new, old = outs
    if isinstance(new, dict):
        assert new.keys() == old.keys()
        for k in new:
            assert np.array_equal(new[k], old[k], equal_nan=True), f"{k} differs between the routes"
    else:
        for a, b in zip(new, old):
            assert np.array_equal(a, b, equal_nan=True)
    return new


def _extend_ctx(pts, sph, dim=3):
    ctx = Context(dim, node_capacity=len(pts))
    ctx.nodes_append(pts)
    if sph is not None:
        ctx.spheres_set(sph)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    return ctx


def test_full_size_c4(oracle):
    N, M, B = 200_000, 256, 16_384
    pts, Q, sph = synth.nodes(N, 3), synth.queries(B, 3), synth.spheres(M)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        assert out["offsets"][-1] > 10 * B
    _vs_oracle(oracle, out, pts, Q, r, oracle.make_spheres(sph), label="C4: ")
    print(f"\ntile placement C4: {B} samples, {len(out['idx'])} entries against the oracle")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 255, 4097, 16_384, 131_072])
def test_batch_sizes(oracle, B):
    N = 60_000
    pts, Q, sph = synth.nodes(N, 3), synth.queries(B, 3, seed=B), synth.spheres(64)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        sel = None
        if B > 16_384:
            ctx.set_option(_capi.RRTX_OPT_NN_CULL, 0)
            brute = ctx.extend_candidates(Q, r, ROBOT_RADIUS)
            assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == 0
            oracle.assert_same_results(out, brute, EXTEND_FIELDS, label=f"B = {B}, culled vs unculled: ")
            sel = _spread_tiles(B)
            assert len(sel) >= 16_384 and sel[-1] == B - 1
    ref = _vs_oracle(oracle, out, pts, Q, r, oracle.make_spheres(sph), sel, label=f"B = {B}: ")
    assert len(ref["idx"]) >= 5 * len(ref["offsets"][:-1])
    print(f"\ntile placement B = {B}: {len(ref['offsets']) - 1} samples, {len(ref['idx'])} entries against the oracle")


@pytest.mark.parametrize("B", [4096, 131_072])
def test_all_samples_identical_spill(oracle, B):
    N = 60_000
    pts, sph = synth.nodes(N, 3), synth.spheres(64)
    Q = np.repeat(synth.queries(1, 3), B, axis=0)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        d = np.diff(out["offsets"])
        assert np.all(d == d[0])
    # every sample sits in one bucket: every list must be the oracle's one list
    assert (Q == Q[0]).all()
    one = oracle.extend_candidates_batch(_trees(oracle, pts), Q[:1], r, pts, oracle.make_spheres(sph), ROBOT_RADIUS)
    assert len(one["idx"]) > 5
    oracle.assert_same_results(out, oracle.take_samples(one, np.zeros(B, dtype=np.int64)), EXTEND_FIELDS,
                               label=f"{B} identical samples: ")


def test_half_samples_at_one_point(oracle):
    N, B = 60_000, 8192
    pts, sph = synth.nodes(N, 3), synth.spheres(64)
    Q = synth.queries(B, 3)
    Q[::2] = Q[0]
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
    _vs_oracle(oracle, out, pts, Q, r, oracle.make_spheres(sph), label="half the samples at one point: ")


def test_non_finite_and_outside_samples(oracle):
    N, B = 60_000, 2048
    pts, sph = synth.nodes(N, 3), synth.spheres(64)
    Q = synth.queries(B, 3)
    Q[1, 0] = np.nan
    Q[2, 1] = np.inf
    Q[3, 2] = -np.inf
    Q[4] = np.nan
    Q[5:400] *= 3.0                   # outside the tree's bounds
    Q[400:420] = 1e200
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
    # a sample with a NaN coordinate orders against no node: the device answers nearest (INT_MAX, inf) where the
    # reference's kdFindNearest keeps its seed (root, NaN) -- the one field compared on the other samples only
    nan = np.isnan(Q).any(axis=1)
    assert nan.sum() == 2 and (out["nearest_idx"][nan] == 0x7fffffff).all() and np.isinf(out["nearest_dist"][nan]).all()
    fields = tuple(f for f in EXTEND_FIELDS if f not in ("nearest_idx", "nearest_dist"))
    ref = _vs_oracle(oracle, out, pts, Q, r, oracle.make_spheres(sph), label="non-finite / outside samples: ",
                     fields=fields)
    keep = np.flatnonzero(~nan)
    oracle.assert_same_results(oracle.take_samples(out, keep), oracle.take_samples(ref, keep), EXTEND_FIELDS, names=keep,
                               label="non-finite / outside samples: ")
    assert (ref["nearest_idx"][nan] == 0).all() and np.isnan(ref["nearest_dist"][nan]).all()
    assert (np.diff(ref["offsets"]) == 0).sum() > 300                 # the samples outside have empty balls


def test_flat_tree(oracle):
    g = np.arange(-100.0, 100.0, 1.0)
    X, Y = np.meshgrid(g, g)
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], axis=1)
    Q = synth.queries(4096, 3)
    Q[:, 2] = 0.0
    sph = synth.spheres(32)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, 3.0, ROBOT_RADIUS))
    ref = _vs_oracle(oracle, out, pts, Q, 3.0, oracle.make_spheres(sph), label="flat tree: ")
    assert len(ref["idx"]) > 20 * len(Q)


def test_appended_tail_and_sorted_runs(oracle):
    pts = synth.nodes(90_000, 3)
    Q = synth.queries(4096, 3)
    r = synth.ball_radius(len(pts), 3)
    sph = synth.spheres(64)
    ts = oracle.TreeSet(3)
    with Context(3, node_capacity=1024) as ctx:
        ctx.spheres_set(sph)
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
        done = 0
        for upto in (20_000, 20_001, 24_000, 40_000, 90_000):
            ctx.nodes_append(pts[done:upto])
            ts.insert_many(pts[done:upto])
            done = upto
            out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
            ref = oracle.extend_candidates_batch(ts, Q, r, pts[:upto], oracle.make_spheres(sph), ROBOT_RADIUS)
            oracle.assert_same_results(out, ref, EXTEND_FIELDS, label=f"{upto} nodes appended: ")


@pytest.mark.parametrize("dim", [3, 4])
def test_nn_radius(oracle, dim):
    N, B = 60_000, 5000
    pts, Q = synth.nodes(N, dim), synth.queries(B, dim)
    r = synth.ball_radius(N, dim)
    rr = np.random.default_rng(3).uniform(0.0, 2.0 * r, B)
    with _extend_ctx(pts, None, dim) as ctx:
        for radius in (r, rr):
            off, idx, dist = _both_routes(ctx, lambda: ctx.nn_radius(Q, radius))
            ref = oracle.range_batch(_trees(oracle, pts), Q, radius, nearest=False)
            oracle.assert_same_results(dict(offsets=off, idx=idx, key=dist), ref, RANGE_FIELDS,
                                       label=f"nn_radius dim {dim}: ")
    assert (np.diff(ref["offsets"]) == 0).any() and len(ref["idx"]) > 5 * B     # small radii leave some balls empty


def test_polygon_extend_path(oracle):
    N, B = 60_000, 4096
    pts, Q = synth.nodes(N, 3), synth.queries(B, 3)
    r = synth.ball_radius(N, 3)
    polys = synth.polygons(128)
    with _extend_ctx(pts, None) as ctx:
        ctx.polygons_set(polys)
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
    ref = _vs_oracle(oracle, out, pts, Q, r, oracle.PolygonSet(polys), label="polygons: ")
    assert 0.1 < ref["hit_out"].mean() < 0.9


def test_small_batch_several_parts(oracle):
    # 40 samples: three tiles, so several workgroups (parts) share each tile's node list
    N = 60_000
    pts, Q, sph = synth.nodes(N, 3), synth.queries(40, 3), synth.spheres(64)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
    _vs_oracle(oracle, out, pts, Q, r, oracle.make_spheres(sph), label="40 samples: ")
