"""Culled range search without ghosts: the tile kernel places the copies itself from the bucket-slot table the pack
pass fills (three launches), where RRTX_OPT_TUNE bit 4 keeps the place pass (four launches).  Both routes must
return the same arrays, bit for bit, whatever the samples do to the bucket histogram."""
import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

OLD_ROUTE = 4          # RRTX_OPT_TUNE bit: pack -> place -> tile
ROBOT_RADIUS = 0.5


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


def test_full_size_c4():
    N, M, B = 200_000, 256, 16_384
    pts, Q, sph = synth.nodes(N, 3), synth.queries(B, 3), synth.spheres(M)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        assert out["offsets"][-1] > 10 * B


@pytest.mark.parametrize("B", [1, 15, 16, 17, 255, 4097, 16_384, 131_072])
def test_batch_sizes(B):
    N = 60_000
    pts, Q, sph = synth.nodes(N, 3), synth.queries(B, 3, seed=B), synth.spheres(64)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))


@pytest.mark.parametrize("B", [4096, 131_072])
def test_all_samples_identical_spill(B):
    N = 60_000
    pts, sph = synth.nodes(N, 3), synth.spheres(64)
    Q = np.repeat(synth.queries(1, 3), B, axis=0)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        out = _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        d = np.diff(out["offsets"])
        assert np.all(d == d[0])


def test_half_samples_at_one_point():
    N, B = 60_000, 8192
    pts, sph = synth.nodes(N, 3), synth.spheres(64)
    Q = synth.queries(B, 3)
    Q[::2] = Q[0]
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, sph) as ctx:
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))


def test_non_finite_and_outside_samples():
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
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))


def test_flat_tree():
    g = np.arange(-100.0, 100.0, 1.0)
    X, Y = np.meshgrid(g, g)
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], axis=1)
    Q = synth.queries(4096, 3)
    Q[:, 2] = 0.0
    with _extend_ctx(pts, synth.spheres(32)) as ctx:
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, 3.0, ROBOT_RADIUS))


def test_appended_tail_and_sorted_runs():
    pts = synth.nodes(90_000, 3)
    Q = synth.queries(4096, 3)
    r = synth.ball_radius(len(pts), 3)
    with Context(3, node_capacity=1024) as ctx:
        ctx.spheres_set(synth.spheres(64))
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
        done = 0
        for upto in (20_000, 20_001, 24_000, 40_000, 90_000):
            ctx.nodes_append(pts[done:upto])
            done = upto
            _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))


@pytest.mark.parametrize("dim", [3, 4])
def test_nn_radius(dim):
    N, B = 60_000, 5000
    pts, Q = synth.nodes(N, dim), synth.queries(B, dim)
    r = synth.ball_radius(N, dim)
    with _extend_ctx(pts, None, dim) as ctx:
        _both_routes(ctx, lambda: ctx.nn_radius(Q, r))
        rr = np.random.default_rng(3).uniform(0.0, 2.0 * r, B)
        _both_routes(ctx, lambda: ctx.nn_radius(Q, rr))


def test_polygon_extend_path():
    N, B = 60_000, 4096
    pts, Q = synth.nodes(N, 3), synth.queries(B, 3)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, None) as ctx:
        ctx.polygons_set(synth.polygons(128))
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))


def test_small_batch_several_parts():
    # 40 samples: three tiles, so several workgroups (parts) share each tile's node list
    N = 60_000
    pts, Q = synth.nodes(N, 3), synth.queries(40, 3)
    r = synth.ball_radius(N, 3)
    with _extend_ctx(pts, synth.spheres(64)) as ctx:
        _both_routes(ctx, lambda: ctx.extend_candidates(Q, r, ROBOT_RADIUS))
