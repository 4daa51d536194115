"""rrtx_obstacle_release_polygon_batch: removeObstacle's edge loop (R/DRRT.jl:3202-3290, node query :3048-3125) for a
burst of expiring polygon obstacles in one call, and rrtx_polygons_set_active, the flag flip that follows it (:3287).
The reference is the oracle -- sweep_edges_batch(remove=True) in C under the burst's flags (the other listed positions
not in use), remove_obstacle_edges on the lattice scenes; the single call rrtx_obstacle_sweep_polygon(mode 1) on a second
context whose other listed positions are switched off through rrtx_polygons_set_active is held equal as well.  Every
comparison is np.array_equal.

The scenes are those of test_gpu_obstacle_sweep_polygon.py (same seeds and sizes).  What a scene must contain (shared
edges, edges a staying obstacle holds, empty rows, candidate counts that are no multiple of 64) is asserted on the
oracle's numbers before the device is asked.  Oracle rows are computed once per scene and shared."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import release_polygon_model as M
from rrtqx_3d_amd import _capi, drrt, synth
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from test_gpu_obstacle_sweep_polygon import DELTA, RR, _dubins_tree, _env, _graph

pytestmark = pytest.mark.gpu
PIECEWISE, RUNNING_SUM = _capi.RRTX_TIME_COLUMN_PIECEWISE, _capi.RRTX_TIME_COLUMN_RUNNING_SUM
assert (RR, DELTA) == (M.RR, M.DELTA)

_spec = importlib.util.spec_from_file_location(
    "soak_lattice_sweeps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "soak_lattice_sweeps.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _union(rows):
    return np.unique(np.concatenate(list(rows) + [np.zeros(0, np.int32)])).astype(np.int32)


def _reaching(es, ee, usable, root, n):
    """how many nodes reach root over the usable mirrored edges v -> u (what a cost solve gives a finite rrtLMC)"""
    seen = np.zeros(n, dtype=bool)
    seen[root] = True
    es, ee = es[usable], ee[usable]
    while True:
        new = np.unique(es[seen[ee] & ~seen[es]])
        if len(new) == 0:
            return int(seen.sum())
        seen[new] = True


def _raw(ctx, obstacles, delta, r_min, unblock, cap):
    """the C call itself: (rc, needed, offsets, ids)"""
    obs = np.ascontiguousarray(obstacles, dtype=np.int32)
    off = np.full(len(obs) + 1, -7, dtype=np.int64)
    ids = np.empty(max(cap, 1), dtype=np.int32)
    needed = C.c_int64(-1)
    rc = ctx._lib.rrtx_obstacle_release_polygon_batch(ctx.handle, _capi._ptr(obs), len(obs), RR, delta, r_min, 1 if unblock else 0,
                                                      _capi._ptr(off), _capi._ptr(ids), cap, C.byref(needed))
    return rc, needed.value, off, ids


def _single_rows(ctx, s, entries, r_min=0.0, delta=DELTA):
    """the single mode-1 call per entry on ctx, the other listed positions switched off through polygons_set_active"""
    listed = np.unique(entries)
    rows = {}
    for p in listed:
        ctx.polygons_set_active(listed, 0)
        ctx.polygons_set_active([p], s.active[p])
        rows[int(p)] = ctx.obstacle_sweep_polygon(int(p), RR, delta, r_min=r_min, remove=True)
    ctx.polygons_set_active(listed, s.active[listed])
    return [rows[int(p)] for p in entries]


# ---- scene 1: SimpleEdge, the reference's rand_Disc_3 polygons ---------------------------------------------------------
@pytest.fixture(scope="module")
def simple_scene(oracle):
    s = M.simple_scene(oracle)
    assert s.m == 89
    s.add = s.add_rows(oracle, range(s.m))                          # mode 0 of every position (4 and 30: empty)
    s.union = _union(s.add.values())
    s.blocked = s.union[s.union % 5 != 0]                            # ids with id % 5 == 0 stay unblocked: condition 1
    s.dist = np.ones(len(s.es))
    s.dist[s.blocked] = np.inf

    def context(ne=None, blocked=None):
        ctx = Context(3)
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, active=s.active)
        assert ctx.graph_edges_append(s.es[:ne], s.ee[:ne]) == 0
        ctx.graph_edges_block(s.blocked if blocked is None else blocked)
        return ctx
    s.context = context
    return s


def test_simple_edges_two_groups_shuffled(oracle, simple_scene):
    """89 entries, groups of 64 + 25: every position but one in-use one, 4 and 30 (not in use) among them, and one in-use
    position a second time; cap = 8 first"""
    s = simple_scene
    in_use = np.flatnonzero(s.active)
    # the position that stays: the in-use one whose mode-0 row shares most blocked edges with the other rows
    shared = {int(p): int(np.isin(s.add[int(p)], _union(s.add[int(q)] for q in in_use if q != p)).sum()) for p in in_use}
    keep = max(shared, key=lambda p: (np.isin(s.add[p], s.blocked).sum() > 0) * shared[p])
    twice = int(in_use[in_use != keep][11])
    entries = np.array([p for p in range(s.m) if p != keep] + [twice], dtype=np.int32)
    np.random.default_rng(89).shuffle(entries)
    assert len(entries) == 89 and 4 in entries and 30 in entries and keep not in entries
    want = s.burst_rows(oracle, entries, s.dist)
    total = sum(len(w) for w in want)
    leaving_hits = _union(s.add[int(p)] for p in entries)
    free_hit = s.union[s.union % 5 == 0]
    assert np.isin(free_hit, leaving_hits).any()                    # an unblocked edge collides with a leaving obstacle
    assert not np.isin(free_hit, _union(want)).any()
    counts = np.bincount(np.concatenate(want), minlength=len(s.es))
    assert (counts >= 2).sum() > 100                                # some edge is in two or more rows
    held = np.intersect1d(np.intersect1d(s.blocked, leaving_hits), s.add[keep])
    assert len(held) > 0 and not np.isin(held, _union(want)).any()  # a blocked edge hits a leaving and the staying obstacle
    assert any(len(w) == 0 for w in want) and total > 5000
    cand, per_group = s.candidates(oracle, entries, s.dist)
    assert len(per_group) == 2 and min(per_group) > 0
    with s.context() as ctx, s.context() as ctx2:
        rc, needed, off, _ = _raw(ctx, entries, DELTA, 0.0, False, 8)             # the two-call path by hand ...
        assert rc == _capi.RRTX_E_CAPACITY and needed == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        off, ids = ctx.obstacle_release_polygon_batch(entries, RR, DELTA, cap=8)    # ... and through the binding
        rows = _rows_of(off, ids)
        assert ctx.stats().last_sweep_candidates == cand
        single = _single_rows(ctx2, s, entries)
        for j, p in enumerate(entries):
            assert np.array_equal(rows[j], want[j]), (j, p)
            assert np.array_equal(rows[j], single[j]), (j, p)
        a, b = np.flatnonzero(entries == twice)
        assert np.array_equal(rows[a], rows[b]) and len(rows[a]) > 0
        for p in (4, 30):
            assert len(rows[int(np.flatnonzero(entries == p)[0])]) == 0


@pytest.mark.parametrize("ne", [1023, 1024, 1025, 2049])
def test_group_and_block_boundaries(oracle, simple_scene, ne):
    """63, 64 and 65 entries over a mirror cut to one edge short of a block of 1024 edges, a block, one edge more, and
    two blocks and one edge; the positions not listed stay"""
    s = simple_scene
    order = np.random.default_rng(64).permutation(s.m).astype(np.int32)
    blocked = s.blocked[s.blocked < ne]
    dist = s.dist[:ne]
    odd = False
    with s.context(ne, blocked) as ctx:
        for k in (63, 64, 65):
            entries = order[:k]
            want = s.burst_rows(oracle, entries, dist)
            assert sum(len(w) for w in want) > 0
            cand, per_group = s.candidates(oracle, entries, dist)
            odd = odd or any(c % 64 != 0 for c in per_group)
            rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, RR, DELTA))
            assert ctx.stats().last_sweep_candidates == cand
            for j in range(k):
                assert np.array_equal(rows[j], want[j]), (k, j)
    assert odd                                    # some group's candidate count is no multiple of the wave width


def test_stay_range_ends(oracle, simple_scene):
    s = simple_scene
    in_use = np.flatnonzero(s.active).astype(np.int32)
    with s.context() as ctx:
        def check(entries):
            entries = np.asarray(entries, dtype=np.int32)
            want = s.burst_rows(oracle, entries, s.dist)
            rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, RR, DELTA))
            for j in range(len(entries)):
                assert np.array_equal(rows[j], want[j]), (entries.tolist(), j)
            return rows
        # every in-use position leaves: no stay range, every blocked colliding candidate comes back
        rows = check(in_use)
        for j, p in enumerate(in_use):
            assert np.array_equal(rows[j], np.intersect1d(s.add[int(p)], s.blocked))
        assert np.array_equal(_union(rows), s.blocked)
        # the first and the last packed position: one range between them
        rows = check([in_use[0], in_use[-1]])
        assert sum(len(r) for r in rows) > 0
        # two neighbouring packed positions (3 and 5: position 4 is not in use), 10 and 11: an empty range between them
        assert s.active[3] and not s.active[4] and s.active[5]
        rows = check([5, 3, 10, 11])
        assert sum(len(r) for r in rows) > 0
        # only positions that are not in use: empty rows, and unblock has nothing to free
        before = _rows_of(*ctx.obstacle_release_polygon_batch(in_use, RR, DELTA))
        off, ids = ctx.obstacle_release_polygon_batch([4, 30, 4], RR, DELTA, unblock=True)
        assert np.array_equal(off, np.zeros(4, dtype=np.int64)) and len(ids) == 0
        assert ctx.stats().last_sweep_candidates == 0
        after = _rows_of(*ctx.obstacle_release_polygon_batch(in_use, RR, DELTA))
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    with s.context(blocked=np.zeros(0, np.int32)) as ctx:            # a mirror in which nothing is blocked
        off, ids = ctx.obstacle_release_polygon_batch(np.arange(s.m), RR, DELTA, unblock=True)
        assert np.array_equal(off, np.zeros(s.m + 1, dtype=np.int64)) and len(ids) == 0
        assert ctx.stats().last_sweep_candidates == 0


# ---- scene 4: Dubins, static polygons ------------------------------------------------------------------------------------
R_MIN = 1.0


@pytest.fixture(scope="module")
def dubins_scene(oracle):
    polys = [np.array(p) for p in _env()["rand_Disc_3_polygons"]][:40]
    rng = np.random.default_rng(11)
    pts, tree = _dubins_tree(oracle, rng, 1400, 20.0)
    es, ee = _graph(oracle, tree, pts, 4.0, rng, n_long=60)
    active = np.ones(len(polys), dtype=np.uint8)
    active[9] = 0
    s = M.make_scene(oracle, pts, tree, es, ee, polys, active, edge=oracle.EDGE_DUBINS, r_min=R_MIN)
    s.add = s.add_rows(oracle, range(s.m))
    s.union = _union(s.add.values())
    s.blocked = s.union[s.union % 5 != 0]
    s.cost = None

    def context():
        ctx = Context(4)
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, active=active)
        ctx.graph_edges_append(es, ee)
        cost, _ = ctx.dubins_steer(pts[es], pts[ee], R_MIN)
        ctx.graph_edges_set_dist(0, cost)
        ctx.graph_edges_block(s.blocked)
        if s.cost is None:
            s.cost = cost
            s.dist = np.where(np.isin(np.arange(len(es)), s.blocked), np.inf, cost)
        return ctx
    s.context = context
    return s


def test_dubins_edges_static_polygons(oracle, dubins_scene):
    """40 entries drawn from 30 positions (ten stay) in one group, then 70 entries drawn from 34 positions, the one not in
    use among them: a second group in the Dubins check; cap = 8 first"""
    s = dubins_scene
    assert len(s.union) > 500 and len(s.add[9]) == 0
    rng = np.random.default_rng(70)
    perm = rng.permutation(s.m)
    forty = np.concatenate([perm[:30], rng.choice(perm[:30], 10)]).astype(np.int32)
    pool = np.unique(np.concatenate([perm[:33], [9]]))
    seventy = np.concatenate([pool, rng.choice(pool, 70 - len(pool))]).astype(np.int32)
    rng.shuffle(forty)
    rng.shuffle(seventy)
    with s.context() as ctx, s.context() as ctx2:
        for entries in (forty, seventy):
            want = s.burst_rows(oracle, entries, s.dist)
            total = sum(len(w) for w in want)
            stays = np.setdiff1d(np.flatnonzero(s.active), entries)
            held = np.intersect1d(np.intersect1d(s.blocked, _union(s.add[int(p)] for p in entries)), _union(s.add[int(p)] for p in stays))
            assert total > 100 and len(held) > 0 and not np.isin(held, _union(want)).any()
            rc, needed, off, _ = _raw(ctx, entries, DELTA, R_MIN, False, 8)
            assert rc == _capi.RRTX_E_CAPACITY and needed == total
            assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
            rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=R_MIN, cap=8))
            assert ctx.stats().last_sweep_candidates == s.candidates(oracle, entries, s.dist)[0]
            single = _single_rows(ctx2, s, entries, r_min=R_MIN)
            for j, p in enumerate(entries):
                assert np.array_equal(rows[j], want[j]), (j, p)
                assert np.array_equal(rows[j], single[j]), (j, p)


# ---- 5: Dubins with time, moving obstacles ----------------------------------------------------------------------------------
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
    s = M.make_scene(oracle, pts, tree, es, ee, polys, active, kinds=kinds, paths=paths, edge=oracle.EDGE_DUBINS_TIME,
                     r_min=synth.R_MIN_TIME, has_time=True)
    s.moving = [j for j in range(m) if kinds[j] in (6, 7)]
    s.static = [j for j in range(m) if kinds[j] == 3]
    s.add = s.add_rows(oracle, s.moving)
    s.blocked = _union(s.add.values())
    s.dist = np.ones(len(es))
    s.dist[s.blocked] = np.inf

    def context(column):
        ctx = Context(4)
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys, kinds=kinds, paths=paths, active=active)
        ctx.set_space_has_time(True)
        ctx.set_dubins_time_column(column)
        ctx.graph_edges_append(es, ee)
        ctx.graph_edges_block(s.blocked)
        return ctx
    s.context = context
    return s


@pytest.mark.parametrize("column", [PIECEWISE, RUNNING_SUM])
def test_dubins_edges_with_time_moving_obstacles(oracle, moving_scene, column):
    """every second moving position and a repeat leave, the others stay, under both forms of the time column: the single
    call is held equal under both, the oracle's rows under the piecewise form (the form they are written in)"""
    s = moving_scene
    assert len(s.moving) >= 8 and len(s.static) > 0 and len(s.blocked) > 100
    entries = np.array(s.moving[::2] + [s.moving[2]], dtype=np.int32)
    want = s.burst_rows(oracle, entries, s.dist)
    assert sum(len(w) for w in want) > 20
    with s.context(column) as ctx, s.context(column) as ctx2:
        # the static kinds would fail the single call's validation in this space: they take no part in the flag flips
        rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=s.r_min))
        single = _single_rows(ctx2, s, entries, r_min=s.r_min)
        for j, p in enumerate(entries):
            assert np.array_equal(rows[j], single[j]), p
            if column == PIECEWISE:
                assert np.array_equal(rows[j], want[j]), p
        assert sum(len(r) for r in rows) > 20
        # one static position among them: the reference's error for the whole call, and nothing is unblocked
        bad = entries[:2].tolist() + [s.static[0]] + entries[2:].tolist()
        rc, _, off, _ = _raw(ctx, bad, DELTA, s.r_min, True, 1 << 16)
        assert rc == _capi.RRTX_E_STATE and np.all(off == -7)
        again = _rows_of(*ctx.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=s.r_min))
        assert all(np.array_equal(a, b) for a, b in zip(rows, again))


# ---- 6: unblock ----------------------------------------------------------------------------------------------------------------
def test_unblock_in_the_call_is_unblock_over_the_union(oracle, dubins_scene):
    """Scene 4, root 0, twin contexts: unblock=True against the same call without it plus rrtx_graph_edges_unblock of the
    union, through graph_cost_update"""
    s = dubins_scene
    entries = np.array([12, 3, 20, 0, 33, 21, 7, 13, 3], dtype=np.int32)
    with s.context() as c1, s.context() as c2:
        want = s.burst_rows(oracle, entries, s.dist)
        union = _union(want)
        total = sum(len(w) for w in want)
        assert len(union) > 0 and total > len(union)                 # some edge is in two rows
        l1, p1, _ = c1.graph_cost_to_root(0)
        l2, p2, _ = c2.graph_cost_to_root(0)
        assert np.array_equal(l1, l2) and np.array_equal(p1, p2)
        # a call that fails unblocks nothing: one id short of room, unblock asked for; the next call returns the same rows
        rc, needed, off, _ = _raw(c1, entries, DELTA, R_MIN, True, total - 1)
        assert rc == _capi.RRTX_E_CAPACITY and needed == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, l1) and np.array_equal(par, p1)
        rows = _rows_of(*c1.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=R_MIN, unblock=True, cap=total))
        for j in range(len(entries)):
            assert np.array_equal(rows[j], want[j]), j
        rows2 = _rows_of(*c2.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=R_MIN))
        assert all(np.array_equal(a, b) for a, b in zip(rows, rows2))
        c2.graph_edges_unblock(_union(rows2))
        l1, p1, _ = c1.graph_cost_update(0)
        l2, p2, _ = c2.graph_cost_update(0)
        assert np.array_equal(l1, l2) and np.array_equal(p1, p2) and not np.array_equal(l1, lmc)
        # what was freed is no longer blocked: a second release finds none of it
        dist = s.dist.copy()
        dist[union] = s.cost[union]
        want2 = s.burst_rows(oracle, entries, dist)
        for c in (c1, c2):
            again = _rows_of(*c.obstacle_release_polygon_batch(entries, RR, DELTA, r_min=R_MIN))
            assert not np.isin(_union(again), union).any()
            assert all(np.array_equal(a, b) for a, b in zip(again, want2))


# ---- 7: the reference's sequence -----------------------------------------------------------------------------------------------
def test_sequence_equality_on_a_mirror_without_long_edges(oracle, simple_scene):
    """the mirror cut to edges no longer than DELTA (the planner's invariant), every colliding edge blocked: twelve single
    mode-1 calls, each followed by graph_edges_unblock and polygons_set_active(j, 0), against one burst with unblock=1 and
    one polygons_set_active(L, 0)"""
    s = simple_scene
    keep = np.flatnonzero(s.length <= DELTA)
    es, ee = s.es[keep], s.ee[keep]
    short = M.make_scene(oracle, s.pts, s.tree, es, ee, s.polys, s.active)
    blocked = _union(short.add_rows(oracle, range(s.m)).values())
    L = np.random.default_rng(12).permutation(np.flatnonzero(s.active))[:12].astype(np.int32)
    dist0 = np.ones(len(es))
    dist = dist0.copy()
    dist[blocked] = np.inf
    want_union = _union(short.burst_rows(oracle, L, dist))
    assert len(want_union) > 500 and np.array_equal(want_union, _union(short.sequence_rows(oracle, L, dist, dist0)))
    # a root outside every obstacle's reach, which more nodes reach once the burst's edges are free
    root = int(np.flatnonzero(~np.isin(np.arange(len(s.pts)), np.r_[es[blocked], ee[blocked]]))[0])
    usable = dist != np.inf
    before = _reaching(es, ee, usable, root, len(s.pts))
    usable[want_union] = True
    assert 100 < before < _reaching(es, ee, usable, root, len(s.pts))

    def context():
        ctx = Context(3)
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, active=s.active)
        assert ctx.graph_edges_append(es, ee) == 0
        ctx.graph_edges_block(blocked)
        return ctx
    with context() as c1, context() as c2:
        la, pa, _ = c1.graph_cost_to_root(root)
        lb, pb, _ = c2.graph_cost_to_root(root)
        assert np.array_equal(la, lb)
        freed = []
        for p in L:
            ids = c1.obstacle_sweep_polygon(int(p), RR, DELTA, remove=True)
            c1.graph_edges_unblock(ids)
            c1.polygons_set_active([p], [0])
            freed.append(ids)
        off, ids = c2.obstacle_release_polygon_batch(L, RR, DELTA, unblock=True)
        c2.polygons_set_active(L, np.zeros(len(L), dtype=np.uint8))
        assert np.array_equal(_union(freed), _union([ids])) and np.array_equal(_union([ids]), want_union)
        l1, p1, _ = c1.graph_cost_update(root)
        l2, p2, _ = c2.graph_cost_update(root)
        assert np.array_equal(l1, l2) and np.array_equal(p1, p2) and not np.array_equal(l1, la)
        # and the two contexts are in the same state afterwards: the next removal answers alike
        nxt = int(np.setdiff1d(np.flatnonzero(s.active), L)[0])
        assert np.array_equal(c1.obstacle_sweep_polygon(nxt, RR, DELTA, remove=True), c2.obstacle_sweep_polygon(nxt, RR, DELTA, remove=True))


# ---- 8: the lattice scenes ------------------------------------------------------------------------------------------------------
def test_polygon_release_on_the_lattice(oracle):
    """P: nodes exactly at range, edges along sides and through vertices; at DELTA and DELTA + 2^-30 against
    remove_obstacle_edges under the burst's flags"""
    s = T.polygon_scene(7)
    o = T.check_polygons_release(s)
    assert o["rows"] == 2 * len(T.polygon_release_entries(s)) and o["ids"] > 100


@pytest.mark.parametrize("root_planted", [False, True])
def test_dubins_release_on_the_lattice(oracle, root_planted):
    """D: Dubins nodes planted exactly at range + pi of the polygons centred at the origin"""
    s = T.dubins_scene(5, root_planted=root_planted)
    o = T.check_dubins_release(s)
    assert o["rows"] == 12 and o["ids"] > 100


# ---- 9: the edges of the contract, the mirror names ----------------------------------------------------------------------------
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
        first = _rows_of(*ctx.obstacle_release_polygon_batch([11, 12], RR, DELTA))
        assert sum(len(r) for r in first) > 0
        for bad in ([0, s.m], [-1, 0]):                              # a position outside the list: nothing runs
            rc, _, off, _ = _raw(ctx, bad, DELTA, 0.0, True, 4096)
            assert rc == _capi.RRTX_E_INVALID and np.all(off == -7)
        obs = np.zeros(1, dtype=np.int32)
        off1 = np.zeros(2, dtype=np.int64)
        needed = C.c_int64()
        call = ctx._lib.rrtx_obstacle_release_polygon_batch
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 1, None, None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, None, 1, RR, DELTA, 0.0, 1, _capi._ptr(off1), None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 1, _capi._ptr(off1), None, -1, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 1, RR, DELTA, 0.0, 1, _capi._ptr(off1), None, 5, C.byref(needed)) == _capi.RRTX_E_INVALID
        assert call(ctx.handle, _capi._ptr(obs), 65537, RR, DELTA, 0.0, 1, _capi._ptr(off1), None, 0, C.byref(needed)) == _capi.RRTX_E_INVALID
        again = _rows_of(*ctx.obstacle_release_polygon_batch([11, 12], RR, DELTA))     # the refused calls freed nothing
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        for p in (11, 4):                                            # one entry: the single call's candidates (4: not in use)
            row = _rows_of(*ctx.obstacle_release_polygon_batch([p], RR, DELTA))[0]
            c_batch = ctx.stats().last_sweep_candidates
            assert np.array_equal(row, ctx.obstacle_sweep_polygon(p, RR, DELTA, remove=True))
            assert c_batch == ctx.stats().last_sweep_candidates
        assert c_batch == 0
    tri = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 2.0]])
    with Context(3) as ctx:                                          # a moving obstacle without a path
        ctx.nodes_append(s.pts)
        ctx.polygons_set([tri, tri + 5.0], kinds=[3, 6], active=[1, 0])
        ctx.graph_edges_append(s.es[:4096], s.ee[:4096])
        rc, _, off, _ = _raw(ctx, [0, 1], DELTA, 0.0, True, 4096)
        assert rc == _capi.RRTX_E_STATE and np.all(off == -7)
        assert "no path" in ctx._lib.rrtx_last_error(ctx.handle).decode()


def test_obstacle_release_polygon_batch_through_the_mirror_names():
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
    edges, ends = [], []
    for i in range(600):
        for j in rng.choice(600, 5, replace=False):
            if i != j:
                edges.append(drrt.newEdge(nodes[i], nodes[int(j)], drrt.DubinsEdge))
                ends.append((i, int(j)))
    ends = np.array(ends)
    assert drrt.registerEdges(KD, edges) == 0
    picked = [obs[2], obs[1]]                                        # the two that overlap leave, not in list order
    added = drrt.obstacleSweepPolygonBatch(S, KD, obs, block=True)
    assert sum(len(r) for r in added) > 20
    rows = drrt.obstacleReleasePolygonBatch(S, KD, picked)
    off, ids = KD.ctx.obstacle_release_polygon_batch([drrt._list_position(S, ob) for ob in picked], S.robotRadius, S.delta,
                                                     r_min=S.minTurningRadius)
    assert len(rows) == 2 and sum(len(r) for r in rows) > 10
    for j in range(2):
        assert np.array_equal(rows[j], ids[off[j]:off[j + 1]])
    both = np.intersect1d(added[1], added[2])                        # held by the two that leave, and by them alone:
    stays = KD.ctx.dubins_edges_check_obstacle(pts[ends[both, 0]], pts[ends[both, 1]], S.minTurningRadius, S.robotRadius,
                                               drrt._list_position(S, obs[0]))
    both = both[stays == 0]                                          # (an edge may hit obs[0] from outside its node list)
    assert len(both) > 0 and np.isin(both, rows[0]).all() and np.isin(both, rows[1]).all()     # shared edges are in both rows
    # one at a time the shared edges stay blocked: the other obstacle is still in use
    alone = drrt.obstacleSweep(S, KD, obs[2], remove=True)
    assert not np.isin(both, alone).any() and set(alone.tolist()) < set(rows[0].tolist())
    assert drrt.obstacleReleasePolygonBatch(S, KD, []) == []
    with pytest.raises(Exception):
        drrt.obstacleReleaseBatch(S, KD, picked)                      # the sphere call keeps refusing polygons


# ---- 10: rrtx_polygons_set_active -------------------------------------------------------------------------------------------------
def test_polygons_set_active_equals_a_fresh_list(oracle, simple_scene, moving_scene):
    s = simple_scene
    flags = s.active.copy()
    flags[[4, 7, 8, 9, 50, 88]] = [1, 0, 0, 0, 0, 0]
    rng = np.random.default_rng(3)
    sel = rng.choice(len(s.es), 3000, replace=False)
    p0, p1 = s.pts[s.es[sel]], s.pts[s.ee[sel]]
    with s.context() as flipped, Context(3) as fresh:
        fresh.nodes_append(s.pts)
        fresh.polygons_set(s.polys, active=flags)
        fresh.graph_edges_append(s.es, s.ee)
        fresh.graph_edges_block(s.blocked)
        flipped.obstacle_sweep_polygon(7, RR, DELTA)                 # (the device tables exist before the flip)
        flipped.polygons_set_active([4, 7, 8, 9, 50, 88, 7], [1, 1, 0, 0, 0, 0, 0])      # 7 twice: the last value wins
        ha, fa = flipped.edges_check(p0, p1, RR, kind=1)
        hb, fb = fresh.edges_check(p0, p1, RR, kind=1)
        assert np.array_equal(ha, hb) and np.array_equal(fa, fb) and ha.any()
        ua, _ = flipped.points_check(p0, RR, kind=1)
        ub, _ = fresh.points_check(p0, RR, kind=1)
        assert np.array_equal(ua, ub) and ua.any()
        for p in (4, 7, 10, 51):
            for remove in (False, True):
                assert np.array_equal(flipped.obstacle_sweep_polygon(p, RR, DELTA, remove=remove),
                                      fresh.obstacle_sweep_polygon(p, RR, DELTA, remove=remove)), (p, remove)
        assert len(flipped.obstacle_sweep_polygon(4, RR, DELTA)) > 0 and len(flipped.obstacle_sweep_polygon(7, RR, DELTA)) == 0
        # errors: a position out of range changes nothing
        with pytest.raises(RrtxError) as ei:
            flipped.polygons_set_active([10, s.m], [0, 0])
        assert ei.value.code == _capi.RRTX_E_INVALID
        with pytest.raises(RrtxError):
            flipped.polygons_set_active([-1], [1])
        assert np.array_equal(flipped.obstacle_sweep_polygon(10, RR, DELTA), fresh.obstacle_sweep_polygon(10, RR, DELTA))
        assert len(fresh.obstacle_sweep_polygon(10, RR, DELTA)) > 0
        flipped.polygons_set_active([], [])                          # k == 0
    # the Dubins check with time: the paths survive the flip
    mvs = moving_scene
    mflags = mvs.active.copy()
    off = [mvs.moving[1], mvs.moving[4]]
    mflags[off] = 0
    sel = rng.choice(len(mvs.es), 1500, replace=False)
    a, b = mvs.pts[mvs.es[sel]], mvs.pts[mvs.ee[sel]]
    moving_only = np.zeros(mvs.m, dtype=np.uint8)
    moving_only[mvs.moving] = 1
    with mvs.context(PIECEWISE) as flipped, Context(4) as fresh:
        fresh.set_wrap(3, 2.0 * math.pi)
        fresh.nodes_append(mvs.pts)
        fresh.polygons_set(mvs.polys, kinds=mvs.kinds, paths=mvs.paths, active=mflags)
        fresh.set_space_has_time(True)
        fresh.set_dubins_time_column(PIECEWISE)
        fresh.graph_edges_append(mvs.es, mvs.ee)
        fresh.graph_edges_block(mvs.blocked)
        flipped.polygons_set_active(off, 0)
        ra = flipped.dubins_edges_check(a, b, mvs.r_min, RR)
        rb = fresh.dubins_edges_check(a, b, mvs.r_min, RR)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)
        p = mvs.moving[0]
        for remove in (False, True):
            assert np.array_equal(flipped.obstacle_sweep_polygon(p, RR, DELTA, r_min=mvs.r_min, remove=remove),
                                  fresh.obstacle_sweep_polygon(p, RR, DELTA, r_min=mvs.r_min, remove=remove))
        flipped.polygons_set_active(off, 1)                          # and back: the paths are still there
        assert len(flipped.obstacle_sweep_polygon(off[0], RR, DELTA, r_min=mvs.r_min)) == len(mvs.add[off[0]])
