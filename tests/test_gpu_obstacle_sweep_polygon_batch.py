"""rrtx_obstacle_sweep_polygon_batch: addNewObstacle's edge loop (R/DRRT.jl:3127-3200, node query :3048-3125) for a
burst of polygon obstacles in one call.  The reference is the oracle, oracle.add_new_obstacle_edges per row; the single
call rrtx_obstacle_sweep_polygon on the same context is held equal as well.  Every comparison is np.array_equal.

The scenes are those of test_gpu_obstacle_sweep_polygon.py (same seeds and sizes), so the oracle's rows are known not
to be trivial; what a scene must contain (totals, shared edges, candidate counts that are no multiple of 64) is asserted
on the oracle's numbers.  Oracle rows are computed once per scene and shared."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, drrt, synth
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from test_gpu_obstacle_sweep_polygon import DELTA, RR, _dubins_tree, _env, _graph

pytestmark = pytest.mark.gpu
PIECEWISE, RUNNING_SUM = _capi.RRTX_TIME_COLUMN_PIECEWISE, _capi.RRTX_TIME_COLUMN_RUNNING_SUM


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _raw(ctx, obstacles, delta, r_min, block, cap):
    """the C call itself: (rc, needed, offsets, ids)"""
    obs = np.ascontiguousarray(obstacles, dtype=np.int32)
    off = np.full(len(obs) + 1, -7, dtype=np.int64)
    ids = np.empty(max(cap, 1), dtype=np.int32)
    needed = C.c_int64(-1)
    rc = ctx._lib.rrtx_obstacle_sweep_polygon_batch(ctx.handle, _capi._ptr(obs), len(obs), RR, delta, r_min, 1 if block else 0,
                                                    _capi._ptr(off), _capi._ptr(ids), cap, C.byref(needed))
    return rc, needed.value, off, ids


def _candidates(s, entries, ne):
    """what last_sweep_candidates must say: per group of 64 entries the mirrored edges (of the first ne) that start at a
    node some in-use obstacle of the group is in conflict with, summed over the groups -- from the oracle's node lists"""
    total = 0
    for g0 in range(0, len(entries), 64):
        nodes = set()
        for p in entries[g0:g0 + 64]:
            if s.active[p]:
                nodes |= s.nodes(int(p))
        total += int(np.isin(s.es[:ne], np.fromiter(nodes, dtype=np.int64, count=len(nodes))).sum())
    return total


# ---- scene 1: SimpleEdge, the reference's rand_Disc_3 polygons (test_simple_edges_discoverable_polygons) ----------------
@pytest.fixture(scope="module")
def simple_scene(oracle):
    polys = [np.array(p) for p in _env()["rand_Disc_3_polygons"]]
    m = len(polys)
    assert m == 89
    rng = np.random.default_rng(5)
    n = 2500
    pts = np.c_[rng.uniform(-20, 20, (n, 2)), np.zeros(n)]
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    es, ee = _graph(oracle, tree, pts, 2.5, rng)
    active = np.ones(m, dtype=np.uint8)
    active[[4, 30]] = 0
    ps = oracle.PolygonSet(polys, active=active)
    s = types.SimpleNamespace(polys=polys, m=m, pts=pts, tree=tree, es=es, ee=ee, active=active, ps=ps)
    s.want = [oracle.add_new_obstacle_edges(tree, pts, es, ee, ps, j, RR, DELTA, dubins=False) for j in range(m)]
    node_sets = {}

    def nodes(j):
        if j not in node_sets:
            node_sets[j] = set(oracle.points_in_conflict_polygon(tree, ps, j, RR, DELTA, False, False).tolist())
        return node_sets[j]

    def context(ne=None):
        ctx = Context(3)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, active=active)
        assert ctx.graph_edges_append(es[:ne], ee[:ne]) == 0
        return ctx
    s.nodes, s.context = nodes, context
    return s


def test_simple_edges_two_groups_shuffled(simple_scene):
    """all 89 positions plus position 7 a second time, shuffled: 90 entries, groups of 64 + 26; cap = 8 first"""
    s = simple_scene
    entries = np.array(list(range(s.m)) + [7], dtype=np.int32)
    np.random.default_rng(90).shuffle(entries)
    assert len(entries) == 90 and not np.array_equal(entries, np.sort(entries))
    total = sum(len(s.want[p]) for p in entries)
    assert sum(len(w) for w in s.want) > 2000 and len(s.want[7]) > 0
    with s.context() as ctx:
        rc, needed, off, _ = _raw(ctx, entries, DELTA, 0.0, False, 8)             # the two-call path by hand ...
        assert rc == _capi.RRTX_E_CAPACITY and needed == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(s.want[p]) for p in entries])]))
        off, ids = ctx.obstacle_sweep_polygon_batch(entries, RR, DELTA, cap=8)     # ... and through the binding
        rows = _rows_of(off, ids)
        assert ctx.stats().last_sweep_candidates == _candidates(s, entries, len(s.es))
        for j, p in enumerate(entries):
            assert np.array_equal(rows[j], s.want[p]), (j, p)
            assert np.array_equal(rows[j], ctx.obstacle_sweep_polygon(int(p), RR, DELTA)), (j, p)
        where = {int(p): [j for j in range(90) if entries[j] == p] for p in (4, 7, 30)}
        assert len(rows[where[4][0]]) == 0 and len(rows[where[30][0]]) == 0        # not in use
        a, b = where[7]
        assert np.array_equal(rows[a], rows[b]) and len(rows[a]) > 0


@pytest.mark.parametrize("ne", [1023, 1024, 1025, 2049])
def test_group_and_block_boundaries(simple_scene, oracle, ne):
    """63, 64 and 65 entries (one group short of full, full, one entry into the second) over a mirror cut to one edge
    short of a block of 1024 edges, a block, one edge more, and two blocks and one edge"""
    s = simple_scene
    es, ee = s.es[:ne], s.ee[:ne]
    order = np.random.default_rng(64).permutation(s.m).astype(np.int32)
    want = {int(p): oracle.add_new_obstacle_edges(s.tree, s.pts, es, ee, s.ps, int(p), RR, DELTA, dubins=False)
            for p in order[:65]}
    assert sum(len(w) for w in want.values()) > 0
    odd = False
    with s.context(ne) as ctx:
        for k in (63, 64, 65):
            entries = order[:k]
            off, ids = ctx.obstacle_sweep_polygon_batch(entries, RR, DELTA)
            cand = _candidates(s, entries, ne)
            assert ctx.stats().last_sweep_candidates == cand
            odd = odd or any(_candidates(s, entries[g0:g0 + 64], ne) % 64 != 0 for g0 in range(0, k, 64))
            for j, row in enumerate(_rows_of(off, ids)):
                assert np.array_equal(row, want[int(entries[j])]), (k, j)
                assert np.array_equal(row, ctx.obstacle_sweep_polygon(int(entries[j]), RR, DELTA)), (k, j)
    assert odd                                    # some group's candidate count is no multiple of the wave width


# ---- 3: the root rule, SimpleEdge (test_simple_edges_tree_off_the_plane_and_root_rule) -------------------------------
def test_root_rule_two_squares_in_one_batch(oracle):
    """square A is centred at the origin and the root lies exactly at its search range (kdFindWithinRange takes the
    root with <=); square B is A moved by 2^-36 away from the root, an exact shift, which puts the root 1.3e-12 of the
    range beyond B's: the root's out-edge is in A's row only.  RRTX_OPT_ROOT_RULE = 0: node 0 is no root."""
    rng = np.random.default_rng(8)
    n = 1500
    sq_a = np.array([[-2.0, -2.0], [2.0, -2.0], [2.0, 2.0], [-2.0, 2.0]])
    shift = 2.0 ** -36
    sq_b = sq_a - np.array([shift, 0.0])
    assert np.array_equal(sq_b[:, 0] + shift, sq_a[:, 0])                      # (the shift is exact)
    rng_range = (RR + DELTA) + math.sqrt(8.0)
    pts = np.c_[rng.uniform(-15, 15, (n, 2)), rng.uniform(-3, 3, n)]
    pts[0] = [rng_range, 0.0, 0.0]
    pts[1] = [0.5, 0.25, 0.0]
    assert 1e-12 < (pts[0, 0] + shift) / rng_range - 1.0 < 2e-12
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    es, ee = _graph(oracle, tree, pts, 3.0, rng)
    ps = oracle.PolygonSet([sq_a, sq_b])
    want = [oracle.add_new_obstacle_edges(tree, pts, es, ee, ps, j, RR, DELTA, dubins=False) for j in (0, 1)]
    root_edge = int(np.nonzero((es == 0) & (ee == 1))[0][0])
    assert root_edge in want[0].tolist() and root_edge not in want[1].tolist() and len(want[1]) > 20
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.polygons_set([sq_a, sq_b])
        ctx.graph_edges_append(es, ee)
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch([0, 1], RR, DELTA))
        for j in (0, 1):
            assert np.array_equal(rows[j], want[j]) and np.array_equal(rows[j], ctx.obstacle_sweep_polygon(j, RR, DELTA))
        assert root_edge in rows[0].tolist() and root_edge not in rows[1].tolist()
        ctx.set_option(_capi.RRTX_OPT_ROOT_RULE, 0)            # (the oracle has no such mode: the single calls are the reference)
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch([0, 1], RR, DELTA))
        for j in (0, 1):
            assert np.array_equal(rows[j], ctx.obstacle_sweep_polygon(j, RR, DELTA))
        assert root_edge not in rows[0].tolist() and np.array_equal(rows[1], want[1])
        assert set(rows[0].tolist()) < set(want[0].tolist())


# ---- scene 4: Dubins, static polygons (test_dubins_edges_static_polygons) ----------------------------------------------
R_MIN = 1.0


@pytest.fixture(scope="module")
def dubins_scene(oracle):
    polys = [np.array(p) for p in _env()["rand_Disc_3_polygons"]][:40]
    m = len(polys)
    rng = np.random.default_rng(11)
    pts, tree = _dubins_tree(oracle, rng, 1400, 20.0)
    es, ee = _graph(oracle, tree, pts, 4.0, rng, n_long=60)
    active = np.ones(m, dtype=np.uint8)
    active[9] = 0
    ps = oracle.PolygonSet(polys, active=active)
    s = types.SimpleNamespace(polys=polys, m=m, pts=pts, tree=tree, es=es, ee=ee, active=active, ps=ps)
    s.want = [oracle.add_new_obstacle_edges(tree, pts, es, ee, ps, j, RR, DELTA, dubins=True, r_min=R_MIN) for j in range(m)]

    def context():
        ctx = Context(4)
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, active=active)
        ctx.graph_edges_append(es, ee)
        cost, _ = ctx.dubins_steer(pts[es], pts[ee], R_MIN)
        ctx.graph_edges_set_dist(0, cost)
        return ctx
    s.context = context
    return s


def test_dubins_edges_static_polygons(dubins_scene):
    """all 40 positions in one group, then 70 entries (every position and 30 repeats): a second group in the Dubins check"""
    s = dubins_scene
    assert sum(len(w) for w in s.want) > 500 and len(s.want[9]) == 0
    rng = np.random.default_rng(70)
    seventy = np.concatenate([np.arange(s.m), rng.integers(0, s.m, 30)]).astype(np.int32)
    rng.shuffle(seventy)
    with s.context() as ctx:
        single = [ctx.obstacle_sweep_polygon(j, RR, DELTA, r_min=R_MIN) for j in range(s.m)]
        for entries in (np.arange(s.m, dtype=np.int32), seventy):
            rows = _rows_of(*ctx.obstacle_sweep_polygon_batch(entries, RR, DELTA, r_min=R_MIN, cap=8))
            assert len(rows) == len(entries)
            for j, p in enumerate(entries):
                assert np.array_equal(rows[j], s.want[p]), (j, p)
                assert np.array_equal(rows[j], single[p]), (j, p)


# ---- 5: Dubins with time, moving obstacles (test_dubins_edges_with_time_moving_obstacles) ----------------------------
@pytest.fixture(scope="module")
def moving_scene(oracle):
    env = _env()
    mv = [np.array(p) for p in env["rand_StaticTime_7_polygons"]][:6]
    mv_paths = [np.array(p) for p in env["rand_StaticTime_7_paths"]][:6]
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(24)
    polys = mv + polys
    kinds = [6, 7, 6, 7, 6, 7] + list(kinds)
    paths = mv_paths + list(paths)
    m = len(polys)
    active = np.ones(m, dtype=np.uint8)
    rng = np.random.default_rng(13)
    pts, tree = _dubins_tree(oracle, rng, 900, 30.0, with_time=True)
    pts[:, 2] = rng.uniform(0.0, 30.0, len(pts))
    tree = oracle.KDTree(4, wraps=[3], wrap_points=[2.0 * math.pi])
    tree.insert_many(pts)
    es, ee = _graph(oracle, tree, pts, 7.0, rng, n_long=60)
    keep = pts[es, 2] > pts[ee, 2]
    es, ee = es[keep], ee[keep]
    ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=active)
    s = types.SimpleNamespace(polys=polys, kinds=kinds, paths=paths, m=m, pts=pts, tree=tree, es=es, ee=ee, active=active, ps=ps,
                              r_min=synth.R_MIN_TIME)
    s.moving = [j for j in range(m) if kinds[j] in (6, 7)]
    s.static = [j for j in range(m) if kinds[j] == 3]
    s.want = {j: oracle.add_new_obstacle_edges(tree, pts, es, ee, ps, j, RR, DELTA, dubins=True, r_min=s.r_min, has_time=True)
              for j in s.moving}

    def context(column):
        ctx = Context(4)
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, kinds=kinds, paths=paths, active=active)
        ctx.set_space_has_time(True)
        ctx.set_dubins_time_column(column)
        ctx.graph_edges_append(es, ee)
        return ctx
    s.context = context
    return s


@pytest.mark.parametrize("column", [PIECEWISE, RUNNING_SUM])
def test_dubins_edges_with_time_moving_obstacles(moving_scene, column):
    """every moving position in one call, under both forms of the time column: the single call is held equal under both,
    the oracle's has_time rows under the piecewise form (the form they are written in, and the one the single call's own
    test compares them under)"""
    s = moving_scene
    assert len(s.moving) >= 8 and len(s.static) > 0 and sum(len(w) for w in s.want.values()) > 100
    with s.context(column) as ctx:
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch(s.moving, RR, DELTA, r_min=s.r_min))
        for j, p in enumerate(s.moving):
            assert np.array_equal(rows[j], ctx.obstacle_sweep_polygon(p, RR, DELTA, r_min=s.r_min)), p
            if column == PIECEWISE:
                assert np.array_equal(rows[j], s.want[p]), p
        assert sum(len(r) for r in rows) > 100
        # one static position among them: the reference's error for the whole call, and nothing is blocked
        lmc0, par0, _ = ctx.graph_cost_to_root(0)
        with pytest.raises(RrtxError) as ei:
            ctx.obstacle_sweep_polygon_batch(s.moving[:3] + [s.static[0]] + s.moving[3:], RR, DELTA, r_min=s.r_min, block=True)
        assert ei.value.code == _capi.RRTX_E_STATE
        lmc, par, _ = ctx.graph_cost_update(0)
        assert np.array_equal(lmc, lmc0) and np.array_equal(par, par0)


# ---- 6: the node sets alone (test_sweep_queries_match_the_kd_tree_node_sets) ----------------------------------------
def test_sweep_queries_match_the_kd_tree_node_sets(oracle):
    """node i's one mirrored edge is i -> i + 1 and a ball that covers the world makes every edge collide: a row of the
    ball IS findPointsInConflictWithObstacle's list for the Dubins query with its ghost"""
    rng = np.random.default_rng(21)
    pts, tree = _dubins_tree(oracle, rng, 3000, 50.0)
    loop = np.arange(len(pts), dtype=np.int32)
    ee = (loop + 1) % len(pts)
    big = np.array([[-500.0, -500.0], [500.0, -500.0], [500.0, 500.0], [-500.0, 500.0]])
    small = np.array([[10.0, 10.0], [14.0, 10.0], [14.0, 13.0]])
    polys, kinds = [small, big, big, big], [3, 1, 1, 1]
    ps = oracle.PolygonSet(polys, kinds=kinds)
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, kinds=kinds)
        ctx.graph_edges_append(loop, ee)
        for delta in (2.0, 8.0, 30.0):
            want = np.sort(oracle.points_in_conflict_polygon(tree, ps, 1, RR, delta, False, True))
            rows = _rows_of(*ctx.obstacle_sweep_polygon_batch([1, 2, 3], RR, delta, r_min=1.0))
            for row in rows:
                assert np.array_equal(row, want) and len(row) > 0
        want_ball = np.sort(oracle.points_in_conflict_polygon(tree, ps, 1, RR, 3.0, False, True))
        want_small = oracle.add_new_obstacle_edges(tree, pts, loop, ee, ps, 0, RR, 3.0, dubins=True, r_min=1.0)
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch([0, 1], RR, 3.0, r_min=1.0))
        assert np.array_equal(rows[1], want_ball) and np.array_equal(rows[0], want_small)
        nodes0 = oracle.points_in_conflict_polygon(tree, ps, 0, RR, 3.0, False, True)
        assert 0 < len(want_small) < len(nodes0) < len(pts) and len(want_small) < len(want_ball)


# ---- 7: block ------------------------------------------------------------------------------------------------------------
def test_block_in_the_call_is_block_over_the_union(dubins_scene):
    """Scene 4, root 0.  Solve, sweep 8 obstacles with block=True, update -- against solve, 8 single sweeps,
    rrtx_graph_edges_block(union), update -- against block first, then a full solve."""
    s = dubins_scene
    order = np.array([12, 3, 20, 0, 33, 21, 7, 13], dtype=np.int32)
    want = [s.want[p] for p in order]
    union = np.unique(np.concatenate(want))
    total = sum(len(w) for w in want)
    assert len(union) > 0 and total > len(union)                     # some edge is in two rows
    with s.context() as c1, s.context() as c2, s.context() as c3:
        lmc0, par0, _ = c1.graph_cost_to_root(0)
        assert np.isin(par0, union).any()                            # a blocked edge is some node's parent edge
        # a call that fails blocks nothing: one id short of room, block asked for
        rc, needed, off, _ = _raw(c1, order, DELTA, R_MIN, True, total - 1)
        assert rc == _capi.RRTX_E_CAPACITY and needed == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, lmc0) and np.array_equal(par, par0)
        # 1: blocked by the batched call
        off, ids = c1.obstacle_sweep_polygon_batch(order, RR, DELTA, r_min=R_MIN, block=True, cap=total)
        for j, row in enumerate(_rows_of(off, ids)):
            assert np.array_equal(row, want[j]), j
        lmc1, par1, _ = c1.graph_cost_update(0)
        # 2: the single calls and one block of the union
        l2, p2, _ = c2.graph_cost_to_root(0)
        assert np.array_equal(l2, lmc0) and np.array_equal(p2, par0)
        got = [c2.obstacle_sweep_polygon(int(p), RR, DELTA, r_min=R_MIN) for p in order]
        for j in range(len(order)):
            assert np.array_equal(got[j], want[j]), j
        c2.graph_edges_block(np.unique(np.concatenate(got)))
        lmc2, par2, _ = c2.graph_cost_update(0)
        # 3: blocked before the first solve
        c3.graph_edges_block(union)
        lmc3, par3, _ = c3.graph_cost_to_root(0)
        assert not np.array_equal(lmc3, lmc0)
        for lmc, par in ((lmc1, par1), (lmc2, par2)):
            assert np.array_equal(lmc, lmc3) and np.array_equal(par, par3)
        # blocked edges do not change what a sweep returns
        off, ids = c1.obstacle_sweep_polygon_batch(order, RR, DELTA, r_min=R_MIN, cap=total)
        assert np.array_equal(ids, np.concatenate(want))


# ---- 8: the edges of the contract ---------------------------------------------------------------------------------------
def test_edges_of_the_contract(simple_scene):
    s = simple_scene
    with Context(3) as ctx:                                          # an empty tree
        ctx.polygons_set(s.polys, active=s.active)
        rc, needed, off, _ = _raw(ctx, [], DELTA, 0.0, False, 0)      # k = 0 comes first
        assert rc == _capi.RRTX_OK and off[0] == 0 and needed == 0
        rc, _, _, _ = _raw(ctx, [0, 1], DELTA, 0.0, False, 16)
        assert rc == _capi.RRTX_E_STATE
        ctx.nodes_append(s.pts)                                      # an empty mirror: k + 1 zero offsets
        rc, needed, off, _ = _raw(ctx, [3, 1, 2], DELTA, 0.0, True, 16)
        assert rc == _capi.RRTX_OK and needed == 0 and np.array_equal(off, np.zeros(4, dtype=np.int64))
    with s.context() as ctx:
        lmc0, par0, _ = ctx.graph_cost_to_root(0)
        for bad in ([0, s.m], [-1, 0]):                              # a position outside the list: nothing runs
            rc, _, off, _ = _raw(ctx, bad, DELTA, 0.0, True, 4096)
            assert rc == _capi.RRTX_E_INVALID and np.all(off == -7)
        obs = np.zeros(1, dtype=np.int32)
        off1 = np.zeros(2, dtype=np.int64)
        needed = C.c_int64()
        call = ctx._lib.rrtx_obstacle_sweep_polygon_batch
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 0, None, None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, None, 1, RR, DELTA, 0.0, 0, _capi._ptr(off1), None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 0, _capi._ptr(off1), None, -1, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 0, _capi._ptr(off1), None, 5, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 65537, RR, DELTA, 0.0, 0, _capi._ptr(off1), None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        lmc, par, _ = ctx.graph_cost_update(0)
        assert np.array_equal(lmc, lmc0) and np.array_equal(par, par0)
        for p in (11, 4):                                            # one entry: the single call's candidates (4: not in use)
            row = _rows_of(*ctx.obstacle_sweep_polygon_batch([p], RR, DELTA))[0]
            c_batch = ctx.stats().last_sweep_candidates
            assert np.array_equal(row, ctx.obstacle_sweep_polygon(p, RR, DELTA))
            assert c_batch == ctx.stats().last_sweep_candidates
        assert c_batch == 0 and len(s.want[11]) > 0
    tri = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 2.0]])
    with Context(3) as ctx:                                          # a moving obstacle without a path
        ctx.nodes_append(s.pts)
        ctx.polygons_set([tri, tri + 5.0], kinds=[3, 6], active=[1, 0])
        ctx.graph_edges_append(s.es[:4096], s.ee[:4096])
        rc, _, off, _ = _raw(ctx, [0, 1], DELTA, 0.0, True, 4096)
        assert rc == _capi.RRTX_E_STATE and np.all(off == -7)
        assert "no path" in ctx._lib.rrtx_last_error(ctx.handle).decode()
        with pytest.raises(RrtxError):
            ctx.obstacle_sweep_polygon(1, RR, DELTA)


# ---- 9: the mirror names ----------------------------------------------------------------------------------------------
def test_obstacle_sweep_polygon_batch_through_the_mirror_names():
    rng = np.random.default_rng(17)
    S = drrt.CSpace(4, -1.0, [-15, -15, 0, 0], [15, 15, 0, 2 * math.pi], [0, 0, 0, 0], [1, 1, 0, 0])
    S.robotRadius, S.delta, S.minTurningRadius, S.spaceHasTheta = 0.5, 6.0, 1.0, True
    KD = drrt.KDTree(4, None, [4], [2.0 * math.pi])
    pts = np.c_[rng.uniform(-15, 15, (600, 2)), np.zeros(600), rng.uniform(0, 2 * math.pi, 600)]
    nodes = [drrt.RRTNode(p) for p in pts]
    for nd in nodes:
        drrt.kdInsert(KD, nd)
    squares = [np.array([[x, y], [x + 3, y], [x + 3, y + 2], [x, y + 2]], dtype=float) for x, y in ((-6, -4), (2, 1), (2.5, 1.5))]
    obs = [drrt.Obstacle(3, sq) for sq in squares]
    for ob in obs:
        ob.obstacleUnused = False
        drrt.listPush(S.obstacles, ob)
    edges = []
    for i in range(600):
        for j in rng.choice(600, 5, replace=False):
            if i != j:
                edges.append(drrt.newEdge(nodes[i], nodes[int(j)], drrt.DubinsEdge))
    assert drrt.registerEdges(KD, edges) == 0
    picked = [obs[2], obs[0], obs[1]]                                # not in list order
    rows = drrt.obstacleSweepPolygonBatch(S, KD, picked)
    assert len(rows) == 3 and sum(len(r) for r in rows) > 20
    for ob, row in zip(picked, rows):
        assert np.array_equal(row, drrt.obstacleSweep(S, KD, ob))
    assert drrt.obstacleSweepPolygonBatch(S, KD, []) == []
    with pytest.raises(Exception):
        drrt.obstacleSweepBatch(S, KD, picked)                        # the sphere call keeps refusing polygons
