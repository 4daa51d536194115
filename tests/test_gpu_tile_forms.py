"""The tile kernel of the culled range search has two forms: the looped one (a workgroup walks tiles tile, tile +
n_slots, ... and lists the tree's chunks in passes of 1 024) and the straight one, compiled without the two loops,
which runs when every workgroup has at most one tile and the tree at most 1 024 chunks.  RRTX_OPT_TUNE value 8 keeps
the looped form everywhere and rrtx_last_tile_form says which one ran (0 none, 1 looped, 2 straight).  Every small
test of the suite runs the straight form, so this file holds the two against each other, bit for bit, on every
instantiation (fused / unfused, slot table / place pass, 3-D / 4-D with ghosts), and walks the two loops of the
looped form that no other small test walks: the tile stride of a capped grid and a second chunk pass.

The tree of most cases: 9 001 uniform nodes in the +-50 box, r = ball_radius(9001, 3) = 8, robot radius 0.5."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

N = 9001
ROBOT_RADIUS = 0.5
LOOP_FORM = 8          # RRTX_OPT_TUNE value: the looped form everywhere
PLACE_PASS = 4         # RRTX_OPT_TUNE value: pack -> place -> tile
LOOPED, STRAIGHT = 1, 2
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")
_CACHE = {}


def _tree():
    if "pts" not in _CACHE:
        _CACHE["pts"] = synth.nodes(N, 3)
        _CACHE["r"] = synth.ball_radius(N, 3)
    return _CACHE["pts"], _CACHE["r"]


def _spheres():
    """64 spheres, sphere 0 moved onto a node of the tree: the edges that end at that node collide"""
    if "sph" not in _CACHE:
        sph = synth.spheres(64)
        sph[0, :3] = _tree()[0][17] + np.array([0.3, 0.0, 0.0])
        _CACHE["sph"] = sph
    return _CACHE["sph"]


def _samples(B):
    """B samples; sample 0 just outside the inflated surface of sphere 0 (safe, one colliding edge), sample 1 at the
    centre of sphere 1 (unsafe).  The first samples of every batch size are the same rows of one draw."""
    if "Q" not in _CACHE:
        sph = _spheres()
        Q = synth.queries(16384, 3, seed=4242)
        Q[0] = sph[0, :3] + np.array([sph[0, 3] + ROBOT_RADIUS + 0.05, 0.0, 0.0])
        Q[1] = sph[1, :3]
        _CACHE["Q"] = Q
    return _CACHE["Q"][:B]


def _reference(oracle):
    """the oracle's extend() preamble for the first 2 500 samples (computed once)"""
    if "ref" not in _CACHE:
        pts, r = _tree()
        trees = oracle.TreeSet(3, pts)
        _CACHE["ref"] = oracle.extend_candidates_batch(trees, _samples(2500), r, pts, oracle.make_spheres(_spheres()),
                                                       ROBOT_RADIUS)
    return _CACHE["ref"]


def _both_values(a):
    a = np.asarray(a)
    return bool((a == 0).any() and (a != 0).any())


def _ctx():
    ctx = Context(3, node_capacity=N)
    ctx.nodes_append(_tree()[0])
    ctx.spheres_set(_spheres())
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    return ctx


def _extend(ctx, Q, r, tune, form, placement, cull=2):
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
    ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
    out = ctx.extend_candidates(Q, r, ROBOT_RADIUS)
    assert ctx.last_tile_form() == form, (tune, cull)
    assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == placement, (tune, cull)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    return out


def _radius(ctx, Q, r, tune, form, cull=2):
    """one range search as dict(offsets, idx, key) with the form it must have run in"""
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
    ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
    offsets, idx, dist = ctx.nn_radius(Q, r)
    assert ctx.last_tile_form() == form, (tune, cull)
    units = ctx.stats().last_scan_units
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    return dict(offsets=offsets, idx=idx, key=dist), units


LIST_FIELDS = ("offsets", "idx", "key")


# ------------------------------------------------------------------------------------------- fused extend route
def test_fused_route_four_ways(oracle):
    """<3, EXT, SL> and <3, EXT, !SL> in both forms: all eight extend fields among the four and against the oracle"""
    _, r = _tree()
    Q = _samples(2500)
    ref = _reference(oracle)
    assert _both_values(ref["hit_out"]) and _both_values(ref["hit_in"]) and _both_values(ref["sample_unsafe"])
    with _ctx() as ctx:
        outs = {}
        for tune, form, placement in ((0, STRAIGHT, 2), (LOOP_FORM, LOOPED, 2), (PLACE_PASS, STRAIGHT, 1),
                                      (PLACE_PASS | LOOP_FORM, LOOPED, 1)):
            outs[tune] = _extend(ctx, Q, r, tune, form, placement)
    for tune, out in outs.items():
        oracle.assert_same_results(out, outs[0], EXTEND_FIELDS, label=f"RRTX_OPT_TUNE {tune} against 0: ")
        oracle.assert_same_results(out, ref, EXTEND_FIELDS, label=f"RRTX_OPT_TUNE {tune}: ")


def test_fused_route_one_part(oracle):
    """16 384 samples: 1 024 tiles, one part each, still one tile per workgroup"""
    _, r = _tree()
    Q = _samples(16384)
    ref = _reference(oracle)
    with _ctx() as ctx:
        new = _extend(ctx, Q, r, 0, STRAIGHT, 2)
        old = _extend(ctx, Q, r, LOOP_FORM, LOOPED, 2)
        two = _extend(ctx, Q, r, 0, 0, 0, cull=0)
    assert _both_values(new["hit_out"]) and _both_values(new["sample_unsafe"])
    oracle.assert_same_results(old, new, EXTEND_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(two, new, EXTEND_FIELDS, label="RRTX_OPT_NN_CULL 0 against 2: ")
    first = np.arange(2500)
    for name, out in (("straight", new), ("looped", old)):
        oracle.assert_same_results(oracle.take_samples(out, first), ref, EXTEND_FIELDS, names=first, label=f"{name}: ")


def test_fused_route_many_parts(oracle):
    """40 samples: 3 tiles (the last one partial), 64 parts each"""
    _, r = _tree()
    Q = _samples(40)
    ref = oracle.take_samples(_reference(oracle), np.arange(40))
    assert _both_values(ref["hit_out"]) and _both_values(ref["sample_unsafe"])
    with _ctx() as ctx:
        new = _extend(ctx, Q, r, 0, STRAIGHT, 2)
        old = _extend(ctx, Q, r, LOOP_FORM, LOOPED, 2)
    oracle.assert_same_results(old, new, EXTEND_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(new, ref, EXTEND_FIELDS, label="straight: ")


# ------------------------------------------------------------------------------------------ unfused range search
@pytest.mark.parametrize("dim,wrapped,tune", [(3, False, 0), (3, False, PLACE_PASS), (4, False, 0), (4, True, 0)])
def test_unfused_radius(oracle, dim, wrapped, tune):
    """rrtx_nn_radius: <3, !EXT, SL>, <3, !EXT, !SL>, <4, !EXT, SL> and, with a wrapped coordinate, <4, !EXT, !SL>
    (ghosts: the number of copies is a device word and the place pass orders them)"""
    pts = synth.nodes(N, dim)
    Q = synth.queries(2500, dim, seed=777)
    r = synth.ball_radius(N, 3)
    wraps, wrap_points = ([3], [2 * math.pi]) if wrapped else (None, None)
    tree = oracle.KDTree(dim, wraps=wraps, wrap_points=wrap_points)
    tree.insert_many(pts)
    ref = oracle.range_batch(tree, Q, r, nearest=False)
    assert ref["offsets"][-1] > 10 * len(Q)
    with Context(dim, node_capacity=N) as ctx:
        if wrapped:
            ctx.set_wrap(3, 2 * math.pi)
        ctx.nodes_append(pts)
        placement = 1 if (wrapped or tune) else 2
        new, _ = _radius(ctx, Q, r, tune, STRAIGHT)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == placement
        old, _ = _radius(ctx, Q, r, tune | LOOP_FORM, LOOPED)
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == placement
    oracle.assert_same_results(old, new, LIST_FIELDS, label="looped against straight: ")
    oracle.assert_same_results(new, ref, LIST_FIELDS, label="straight: ")


def test_capped_grid_walks_the_tile_stride(oracle):
    """65 600 queries are 4 100 tiles on 4 096 workgroups: workgroups 0 .. 3 take a second tile, so the form is the
    looped one whatever RRTX_OPT_TUNE says.  r = 4.7: about four neighbours per query."""
    pts, _ = _tree()
    Q = synth.queries(65600, 3, seed=909)
    r = 4.7
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        got, _ = _radius(ctx, Q, r, 0, LOOPED)
        brute, _ = _radius(ctx, Q, r, 0, 0, cull=0)
    mean = got["offsets"][-1] / len(Q)
    assert 2.0 < mean < 8.0, mean
    oracle.assert_same_results(got, brute, LIST_FIELDS, label="capped grid against RRTX_OPT_NN_CULL 0: ")


def test_second_chunk_pass(oracle):
    """524 288 nodes are 1 024 chunks, one pass: straight.  One node more and the looped form lists the chunks in two
    passes, with the list reset between them."""
    n = 524288
    pts = synth.nodes(n + 1, 3, seed=31337)
    Q = synth.queries(64, 3, seed=606)
    Q[0] = pts[n] + np.array([0.01, 0.0, 0.0])            # the node of the second pass has a query next to it
    r = synth.ball_radius(n, 3)
    with Context(3, node_capacity=n + 1) as ctx:
        ctx.nodes_append(pts[:n])
        a, _ = _radius(ctx, Q, r, 0, STRAIGHT)
        a8, _ = _radius(ctx, Q, r, LOOP_FORM, LOOPED)
        a0, _ = _radius(ctx, Q, r, 0, 0, cull=0)
        ctx.nodes_append(pts[n:])
        b, _ = _radius(ctx, Q, r, 0, LOOPED)
        b0, _ = _radius(ctx, Q, r, 0, 0, cull=0)
    assert a["offsets"][-1] > 10 * len(Q)
    oracle.assert_same_results(a8, a, LIST_FIELDS, label="524 288 nodes, looped against straight: ")
    oracle.assert_same_results(a, a0, LIST_FIELDS, label="524 288 nodes against RRTX_OPT_NN_CULL 0: ")
    oracle.assert_same_results(b, b0, LIST_FIELDS, label="524 289 nodes against RRTX_OPT_NN_CULL 0: ")
    assert n in b["idx"][b["offsets"][0]:b["offsets"][1]] and n not in a["idx"]


def test_entry_slice_drained_mid_screen(oracle):
    """A NaN node makes the bound of the fp32 screen useless (the tree's largest |coordinate| is then NaN and the
    screen passes everything), so every screen step of 64 groups files 64 x 16 = 1 024 entries in the wave's slice of
    1 536: a wave that takes a third step has had at least one full step among its first two (a tile has at most one
    partial unit of groups) and must have drained its slice before it.  16 384 queries are 1 024 full tiles with one
    part each, one tile per workgroup: more than 2 x 4 x 1 024 steps in all means some wave took three.  The nodes
    appended after the index was built are what gives every tile that many steps (their chunks are tested by
    extent)."""
    rng = np.random.default_rng(77)
    n0, nb, steps = 40_000, 6000, 5
    pts = rng.uniform(-50, 50, (n0 + nb * steps, 3))
    pts[n0 + 100] = [np.nan, 0.0, 0.0]                    # a node nothing can find, inside a run
    pts[n0 + 101] = pts[17]                               # a duplicate of an indexed node
    Q = rng.uniform(-50, 50, (16384, 3))
    r = 4.5
    pts_o = pts.copy()
    pts_o[n0 + 100] = 1e9                                 # the oracle's stand-in: as unreachable, keeps indices aligned
    tree = oracle.KDTree(3)
    tree.insert_many(pts_o)
    ref = oracle.range_batch(tree, Q[:500], r, nearest=False)
    assert ref["offsets"][-1] > 10 * 500
    with Context(3) as ctx:
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
        ctx.nodes_append(pts[:n0])
        ctx.nn_radius(Q[:8], r)                           # builds the index
        for s in range(steps):
            ctx.nodes_append(pts[n0 + s * nb:n0 + (s + 1) * nb])
        new, units_new = _radius(ctx, Q, r, 0, STRAIGHT)
        old, units_old = _radius(ctx, Q, r, LOOP_FORM, LOOPED)
    n_waves = 4 * (len(Q) // 16)
    print(f"screen steps: straight {units_new}, looped {units_old}, waves {n_waves}")
    assert units_new > 2 * n_waves and units_old > 2 * n_waves       # the drain happened, in both forms
    oracle.assert_same_results(old, new, LIST_FIELDS, label="looped against straight: ")
    first = dict(offsets=new["offsets"][:501], idx=new["idx"][:new["offsets"][500]], key=new["key"][:new["offsets"][500]])
    oracle.assert_same_results(first, ref, LIST_FIELDS, label="straight, first 500 queries: ")
