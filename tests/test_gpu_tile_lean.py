"""The straight form of the tile kernel after its lean pass ("tile kernel, lean"): the two-level
placement search, the screen that keeps the copy records in vector registers, and the grid description requested
before the reach.  Nothing in the data flow changed, so every output array must still equal, bit for bit,

  * the oracle's,
  * the looped form's (RRTX_OPT_TUNE 8; rrtx_last_tile_form says 2 and 1), which the pass left alone, and
  * the two-kernel route's (RRTX_OPT_NN_CULL 0), which has no tile kernel at all,

on shapes chosen for the code that changed:

  trees    PLAIN: 9 001 uniform nodes in the +-50 box (NN_CULL 2 forces the culled search on a tree this small).
           TAIL: the same, then a batch of 1 100 nodes (>= 1 024: laid out as one sorted run) and five batches of
           1 000 (unsorted tail: ten chunks every tile screens by extent), 15 101 nodes; one node of the tail is NaN,
           which makes the fp32 bound useless, so every screen step fills the wave's slice.
  batches  B = 1, 15, 16, 17, 48 (partial and full tiles), 1 040 (65 tiles, 256 buckets, one counter per thread of
           the placement scan) and 16 384 (1 024 tiles with one part each, all 4 096 buckets, sixteen counters per
           thread; on TAIL every wave takes more than two screen steps and drains its slice between them).
  buckets  48 identical samples (8 buckets, 32 slots each: ranks 32 .. 47 go to the spill list), and 1 040 samples
           of which 300 are identical (20 slots per bucket: 280 spilled), 400 lie in one small cube (few buckets,
           many of the 256 empty) and 340 are spread out.
  flags    the first samples of every batch: one with nine spheres within reach of its ball (more than kSphListCap
           = 8: the full loop), one with eight, one with one, one with none; one equal to a node (a zero-length
           edge), one exactly r away from node 0 along x, one at the centre of a sphere (unsafe).

r = ball_radius(9001, 3) = 8, robot radius 0.5."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

N = 9001
RUN, TAIL_BATCH, TAIL_BATCHES = 1100, 1000, 5
NAN_AT = N + RUN + 2 * TAIL_BATCH + 77           # inside the third unsorted batch
ROBOT_RADIUS = 0.5
LOOP_FORM = 8          # RRTX_OPT_TUNE value: the looped form everywhere
PLACE_PASS = 4         # RRTX_OPT_TUNE value: pack -> place -> tile
LOOPED, STRAIGHT = 1, 2
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")
LIST_FIELDS = ("offsets", "idx", "key")
N_REF = 1040           # samples of the shared batch the oracle is asked about (once per tree)
CLUSTERS = {0: 9, 1: 8, 2: 1}                    # sample -> spheres within reach of its ball
_CACHE = {}


def _r():
    return synth.ball_radius(N, 3)


def _points():
    """all 15 101 nodes in order of arrival (PLAIN is the first 9 001); the oracle gets a far-away stand-in for the
    NaN node, which nothing can find either and which keeps the indices aligned"""
    if "pts" not in _CACHE:
        rng = np.random.default_rng(20240)
        pts = np.concatenate([synth.nodes(N, 3), rng.uniform(-50, 50, (RUN + TAIL_BATCH * TAIL_BATCHES, 3))])
        pts[NAN_AT] = [np.nan, 0.0, 0.0]
        pts[NAN_AT + 1] = pts[17]                 # a duplicate of an indexed node, in the tail
        ref = pts.copy()
        ref[NAN_AT] = 1e9
        _CACHE["pts"], _CACHE["pts_ref"] = pts, ref
    return _CACHE["pts"], _CACHE["pts_ref"]


_CENTRES = np.array([[-30.0, -30.0, -30.0], [30.0, 30.0, 30.0], [30.0, -30.0, 0.0]])


def _spheres():
    """nine, eight and one small spheres 3 away from the first three samples, and four large ones elsewhere"""
    if "sph" not in _CACHE:
        rng = np.random.default_rng(11)
        rows = []
        for s, count in CLUSTERS.items():
            d = rng.normal(size=(count, 3))
            d *= 3.0 / np.linalg.norm(d, axis=1, keepdims=True)
            rows.append(np.concatenate([_CENTRES[s] + d, np.full((count, 1), 0.4)], axis=1))
        rows.append(np.array([[0.0, 0.0, 0.0, 3.0], [-30.0, 30.0, 10.0, 3.5], [10.0, 40.0, -40.0, 2.5], [-5.0, -45.0, 35.0, 3.0]]))
        _CACHE["sph"] = np.concatenate(rows)
    return _CACHE["sph"]


def _samples(B):
    """the first B rows of one draw of 16 384; rows 0 .. 6 are the special samples of the docstring"""
    if "Q" not in _CACHE:
        pts, _ = _points()
        sph = _spheres()
        Q = synth.queries(16384, 3, seed=5151)
        Q[0], Q[1], Q[2] = _CENTRES
        Q[3] = [-40.0, 5.0, -20.0]                # no sphere anywhere near
        Q[4] = pts[123]                           # a zero-length edge
        Q[5] = pts[0] + np.array([_r(), 0.0, 0.0])
        Q[6] = sph[-4, :3]                        # centre of the large sphere at the origin
        # spheres whose inflated surface the sample's ball of candidate edges reaches, with nothing near the limit
        gap = np.linalg.norm(sph[None, :, :3] - Q[:4, None, :], axis=2) - sph[None, :, 3] - ROBOT_RADIUS
        assert not np.any(np.abs(gap - _r()) < 2.0)
        assert list((gap <= _r()).sum(axis=1)) == [9, 8, 1, 0]
        _CACHE["Q"] = Q
    return _CACHE["Q"][:B]


def _n_nodes(tail):
    return len(_points()[0]) if tail else N


def _ctx(tail, spheres=True):
    """a context holding PLAIN or TAIL; the index is built by a first search before TAIL's batches arrive"""
    pts, _ = _points()
    ctx = Context(3, node_capacity=len(pts))
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    if spheres:
        ctx.spheres_set(_spheres())
    ctx.nodes_append(pts[:N])
    if tail:
        ctx.nn_radius(pts[:8], _r())
        ctx.nodes_append(pts[N:N + RUN])
        for k in range(TAIL_BATCHES):
            ctx.nodes_append(pts[N + RUN + k * TAIL_BATCH:N + RUN + (k + 1) * TAIL_BATCH])
    return ctx


def _reference(oracle, tail):
    """the oracle's extend() preamble for the first N_REF samples of the shared batch (once per tree)"""
    key = ("ref", tail)
    if key not in _CACHE:
        nodes = _points()[1][:_n_nodes(tail)]
        trees = oracle.TreeSet(3, nodes)
        _CACHE[key] = oracle.extend_candidates_batch(trees, _samples(N_REF), _r(), nodes, oracle.make_spheres(_spheres()),
                                                     ROBOT_RADIUS)
    return _CACHE[key]


def _extend(ctx, Q, tune, form, placement, cull=2):
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
    ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
    out = ctx.extend_candidates(Q, _r(), ROBOT_RADIUS)
    assert ctx.last_tile_form() == form, (tune, cull)
    assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == placement, (tune, cull)
    units = ctx.stats().last_scan_units
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    return out, units


def _radius(ctx, Q, r, tune, form, cull=2):
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
    ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
    offsets, idx, dist = ctx.nn_radius(Q, r)
    assert ctx.last_tile_form() == form, (tune, cull)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    return dict(offsets=offsets, idx=idx, key=dist)


def _three_routes(oracle, ctx, Q, ref, names=None, tune=0, placement=2):
    """straight, looped and two-kernel route on one batch: equal among themselves and to the oracle's rows `ref`"""
    new, units = _extend(ctx, Q, tune, STRAIGHT, placement)
    old, _ = _extend(ctx, Q, tune | LOOP_FORM, LOOPED, placement)
    two, _ = _extend(ctx, Q, 0, 0, 0, cull=0)
    oracle.assert_same_results(old, new, EXTEND_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(two, new, EXTEND_FIELDS, label="RRTX_OPT_NN_CULL 0 against 2: ")
    if names is None:
        oracle.assert_same_results(new, ref, EXTEND_FIELDS, label="straight against the oracle: ")
    else:
        oracle.assert_same_results(oracle.take_samples(new, names), ref, EXTEND_FIELDS, names=names,
                                   label="straight against the oracle: ")
    return new, units


# --------------------------------------------------------------------------------- fused route, <3, EXT, SL>
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 48, 1040])
def test_batch_sizes(oracle, B, tail):
    ref = oracle.take_samples(_reference(oracle, tail), np.arange(B))
    with _ctx(tail) as ctx:
        new, _ = _three_routes(oracle, ctx, _samples(B), ref)
    if B >= 15:
        both = lambda a: bool((np.asarray(a) == 0).any() and (np.asarray(a) != 0).any())
        assert both(new["hit_out"]) and both(new["hit_in"]) and both(new["sample_unsafe"])
        off, idx = np.asarray(new["offsets"]), np.asarray(new["idx"])
        assert 123 in idx[off[4]:off[5]]                                     # the zero-length edge is an entry
        assert min(off[k + 1] - off[k] for k in range(3)) > 0                # the sphere lists had edges to test


def test_all_buckets_and_drained_slices(oracle):
    """16 384 samples on TAIL: every one of the 4 096 buckets is in use, and with the NaN node every screen step
    files 64 x 16 entries in a slice of 1 536, so a wave that takes a third step (more than 2 x 4 x 1 024 steps in
    all) has drained its slice on the way, through the tile's own emitter with the edge flags"""
    Q = _samples(16384)
    first = np.arange(N_REF)
    with _ctx(True) as ctx:
        new, units = _extend(ctx, Q, 0, STRAIGHT, 2)
        old, units_old = _extend(ctx, Q, LOOP_FORM, LOOPED, 2)
        two, _ = _extend(ctx, Q, 0, 0, 0, cull=0)
    n_waves = 4 * (len(Q) // 16)
    assert units > 2 * n_waves and units_old > 2 * n_waves, (units, units_old, n_waves)
    oracle.assert_same_results(old, new, EXTEND_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(two, new, EXTEND_FIELDS, label="RRTX_OPT_NN_CULL 0 against 2: ")
    oracle.assert_same_results(oracle.take_samples(new, first), _reference(oracle, True), EXTEND_FIELDS, names=first,
                               label="straight against the oracle: ")


def _crowded(B):
    """48: all identical.  1 040: 300 identical, 400 in one cube of side 6, 340 spread out (rows of the shared draw)"""
    Q = _samples(B).copy()
    if B == 48:
        Q[:] = [12.5, -7.25, 3.0]
    else:
        Q[:300] = [12.5, -7.25, 3.0]
        Q[300:700] = np.array([-20.0, 20.0, 5.0]) + np.random.default_rng(3).uniform(-3, 3, (400, 3))
    return Q


@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("B", [48, 1040])
def test_bucket_loads(oracle, B, tail):
    """full buckets, the spill list and empty buckets in front of the placement search"""
    Q = _crowded(B)
    nodes = _points()[1][:_n_nodes(tail)]
    ref = oracle.extend_candidates_batch(oracle.TreeSet(3, nodes), Q, _r(), nodes, oracle.make_spheres(_spheres()),
                                         ROBOT_RADIUS)
    assert ref["offsets"][-1] > 10 * B
    with _ctx(tail) as ctx:
        _three_routes(oracle, ctx, Q, ref)


# --------------------------------------------------------------------------------- the other five instantiations
@pytest.mark.parametrize("B", [17, 1040])
def test_fused_place_pass(oracle, B):
    """<3, EXT, !SL>: the copies come from the place pass; the screen reads its records with scalar loads"""
    ref = oracle.take_samples(_reference(oracle, True), np.arange(B))
    with _ctx(True) as ctx:
        _three_routes(oracle, ctx, _samples(B), ref, tune=PLACE_PASS, placement=1)


@pytest.mark.parametrize("dim,wrapped,tune", [(3, False, 0), (3, False, PLACE_PASS), (4, False, 0), (4, True, 0)])
@pytest.mark.parametrize("B", [17, 1040])
def test_unfused_radius(oracle, B, dim, wrapped, tune):
    """rrtx_nn_radius: <3, !EXT, SL>, <3, !EXT, !SL>, <4, !EXT, SL> and, with a wrapped coordinate, <4, !EXT, !SL>;
    9 001 nodes, then a sorted run of 1 100 and an unsorted batch of 1 000"""
    pts = synth.nodes(N + RUN + TAIL_BATCH, dim, seed=808)
    Q = synth.queries(B, dim, seed=777)
    Q[0] = pts[55]
    r = _r()
    wraps, wrap_points = ([3], [2 * math.pi]) if wrapped else (None, None)
    tree = oracle.KDTree(dim, wraps=wraps, wrap_points=wrap_points)
    tree.insert_many(pts)
    ref = oracle.range_batch(tree, Q, r, nearest=False)
    assert ref["offsets"][-1] > 10 * B
    with Context(dim, node_capacity=len(pts)) as ctx:
        if wrapped:
            ctx.set_wrap(3, 2 * math.pi)
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
        ctx.nodes_append(pts[:N])
        ctx.nn_radius(Q[:1], r)
        ctx.nodes_append(pts[N:N + RUN])
        ctx.nodes_append(pts[N + RUN:])
        placement = 1 if (wrapped or tune) else 2
        new = _radius(ctx, Q, r, tune, STRAIGHT)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == placement
        old = _radius(ctx, Q, r, tune | LOOP_FORM, LOOPED)
        two = _radius(ctx, Q, r, 0, 0, cull=0)
    oracle.assert_same_results(old, new, LIST_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(two, new, LIST_FIELDS, label="RRTX_OPT_NN_CULL 0 against 2: ")
    oracle.assert_same_results(new, ref, LIST_FIELDS, label="straight against the oracle: ")
