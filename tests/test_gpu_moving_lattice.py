"""Obstacles that move in time (kinds 6 / 7) through the C-ABI on the lattice-in-time scenes of
tests/moving_lattice_model.py, against the oracle, everything with == / np.array_equal, NaN rows included:
edges_check and points_check in the plane (edges_polygons_kernel<MOVING>, points_polygons_kernel), the PAIRED form
behind extend_candidates (host and _dev), the Dubins check in a space with time with both time columns (its screens
1a / 2a on the path box), and the sweeps and releases (polygon_sweep_queries, one range query per path segment).
tests/test_moving_lattice_scenes.py shows without a device that the scenes hold the ties, knots and NaNs they are for.

rrtx_edges_check_idx reads the sphere list only, so "only the moving obstacles" is asked of the polygon list through
rrtx_edges_check_dev's range of list positions instead.  The rule orders an edge's ends by time, so for a moving
obstacle q -> node and node -> q are the same test and hit_out == hit_in: the PAIRED form's reverse edge is held to the
oracle, but no scene of moving obstacles can tell it from the forward one."""
import math

import numpy as np
import pytest

import moving_lattice_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
TWO_PI = 2.0 * math.pi


def _set(ctx, s):
    ctx.polygons_set(s.polys, kinds=s.kinds, active=s.active, paths=s.paths)


def _ps(oracle, s, active=None):
    return oracle.PolygonSet(s.polys, kinds=s.kinds, active=s.active if active is None else active, paths=s.paths)


def _one(oracle, s, j):
    return oracle.PolygonSet([s.polys[j]], kinds=[s.kinds[j]], active=[s.active[j]], paths=[s.paths[j]])


def _probes(s):
    """a moving obstacle of every group of 32 list positions, the positions either side of the group borders, an
    inactive one"""
    by_group = {}
    for j in s.moving:
        by_group.setdefault(j // 32, j)
    pick = set(by_group.values()) | {j for j in M.CROWD_MOVING_AT if j < s.m and s.kinds[j] in (6, 7)}
    pick |= {j for j in s.moving if not s.active[j]}
    assert {j // 32 for j in pick} == {j // 32 for j in s.moving}
    return sorted(pick)


@pytest.mark.parametrize("name", list(M.SCENES))
def test_edges_check_on_lattice_scenes(oracle, name):
    torch = pytest.importorskip("torch")
    s = M.scene(name)
    ps = s.polygon_set(oracle)
    rr = s.robot_radius
    ohit, ofirst = oracle.edges_check_batch(ps, s.p0, s.p1, rr)
    with Context(3) as ctx:
        _set(ctx, s)
        hit, first = ctx.edges_check(s.p0, s.p1, rr, kind=1)
        print(f"{name}: {len(hit)} edges, {int(hit.sum())} hit, {int((hit != ohit).sum())} differ from the oracle")
        assert np.array_equal(hit, ohit) and np.array_equal(first, ofirst)
        for j in _probes(s):                                             # explicitEdgeCheck(S, edge, ob): one obstacle
            h, _ = ctx.edges_check(s.p0, s.p1, rr, kind=1, obstacle=j)
            assert np.array_equal(h, oracle.edges_check_batch(_one(oracle, s, j), s.p0, s.p1, rr)[0]), j
        # a range of list positions across a border of 32
        lo, hi = (30, min(s.m, 66)) if s.m > 34 else (1, s.m)
        act = s.active.copy()
        act[:lo] = 0
        act[hi:] = 0
        rhit, rfirst = oracle.edges_check_batch(_ps(oracle, s, act), s.p0, s.p1, rr)
        d0, d1 = torch.from_numpy(s.p0).cuda(), torch.from_numpy(s.p1).cuda()
        dh = torch.zeros(len(s.p0), dtype=torch.uint8, device="cuda")
        df = torch.zeros(len(s.p0), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.edges_check_dev(1, d0.data_ptr(), d1.data_ptr(), len(s.p0), rr, -1, lo, hi, dh.data_ptr(), df.data_ptr())
        ctx.sync()
        assert np.array_equal(dh.cpu().numpy(), rhit) and np.array_equal(df.cpu().numpy(), rfirst)
        if 3 in s.kinds:                                                 # only the moving obstacles: every kind 3 switched off
            act = s.active * np.array([k != 3 for k in s.kinds], dtype=np.uint8)
            ctx.polygons_set(s.polys, kinds=s.kinds, active=act, paths=s.paths)
            hit, first = ctx.edges_check(s.p0, s.p1, rr, kind=1)
            mhit, mfirst = oracle.edges_check_batch(_ps(oracle, s, act), s.p0, s.p1, rr)
            assert np.array_equal(hit, mhit) and np.array_equal(first, mfirst) and 0 < mhit.sum() < ohit.sum()


@pytest.mark.parametrize("name", list(M.SCENES))
def test_points_check_on_lattice_scenes(oracle, name):
    """flag and clearance at row times, before the first row, after the last, at clearance exactly 0; with and without
    the clearance (a list that holds a moving obstacle takes the full kernel either way)"""
    s = M.scene(name)
    ps = s.polygon_set(oracle)
    pts = M.scene_points(s)[:600]
    ounsafe, oclr = oracle.points_check_batch(ps, pts, s.robot_radius)
    with Context(3) as ctx:
        _set(ctx, s)
        unsafe, clr = ctx.points_check(pts, s.robot_radius, kind=1)
        assert np.array_equal(unsafe, ounsafe) and np.array_equal(clr, oclr)
        flag, none = ctx.points_check(pts, s.robot_radius, kind=1, want_clearance=False)
        assert none is None and np.array_equal(flag, ounsafe)
    assert 0 < ounsafe.sum() < len(pts)


EXTEND = {"crowd_33": ((-2, 38, -2, 38, 0, 4), 3.3), "crowd_65": ((-2, 52, -2, 52, 0, 3), 3.9),
          "tangent_0.5": ((-8, 8, -9, 7, 2, 10), 2.4), "knots": ((-10, 14, -10, 14, 2, 12), 2.9)}


@pytest.mark.parametrize("name", list(EXTEND))
def test_extend_candidates_paired_form(oracle, name):
    """rrtx_extend_candidates and _dev in 3-D against a polygon list with moving obstacles: both directed edges of every
    entry (the PAIRED form of edges_polygons_kernel) against the oracle; at most 1500 lattice nodes, 63 samples, an
    entry count that is no multiple of 32, so the tail waves of 32 end in a partial one"""
    torch = pytest.importorskip("torch")
    s = M.scene(name)
    ps = s.polygon_set(oracle)
    box, r = EXTEND[name]
    rng = np.random.default_rng(5)
    lo, hi = np.array(box[0::2]), np.array(box[1::2])
    nodes = np.unique(rng.integers(lo * 4, hi * 4 + 1, (1500, 3)), axis=0) * 0.25
    Q = rng.integers(lo * 4 + 4, hi * 4 - 3, (63, 3)) * 0.25
    ref = oracle.extend_candidates_batch(oracle.TreeSet(3, nodes), Q, r, nodes, ps, s.robot_radius)
    n = len(ref["idx"])
    lens = np.diff(ref["offsets"])
    assert n % 32 != 0 and 20 <= np.median(lens) <= 60 and 0 < ref["hit_out"].sum() < n
    with Context(3) as ctx:
        ctx.nodes_append(nodes)
        _set(ctx, s)
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        out = ctx.extend_candidates(Q, r, s.robot_radius)
        for k in ("offsets", "idx", "cost", "hit_out", "hit_in", "sample_unsafe"):
            assert np.array_equal(out[k], ref[k]), k
        cap = n + 100
        d_q = torch.from_numpy(Q).cuda()
        d_off = torch.empty(len(Q) + 1, dtype=torch.int64, device="cuda")
        d_idx = torch.empty(cap, dtype=torch.int32, device="cuda")
        d_cost = torch.empty(cap, dtype=torch.float64, device="cuda")
        d_ho = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_hi = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_need = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.extend_candidates_dev(d_q.data_ptr(), len(Q), r, s.robot_radius, d_off.data_ptr(), d_idx.data_ptr(),
                                  d_cost.data_ptr(), d_ho.data_ptr(), d_hi.data_ptr(), cap, d_need.data_ptr(), None, None, None)
        ctx.sync()
        assert np.array_equal(d_off.cpu().numpy(), ref["offsets"]) and np.array_equal(d_idx.cpu().numpy()[:n], ref["idx"])
        assert np.array_equal(d_ho.cpu().numpy()[:n], ref["hit_out"]) and np.array_equal(d_hi.cpu().numpy()[:n], ref["hit_in"])
    print(f"{name}: {n} entries, lists {lens.min()}..{lens.max()}, {int(ref['hit_out'].sum())} / {int(ref['hit_in'].sum())} hit out / in")


# ---- Dubins edges in a space with time ---------------------------------------------------------------------------------
def _dubins_sets():
    out = []
    s, S, G, _ = M.dubins_ties()
    out.append(("ties", s, S, G))
    s, S, G, _, _ = M.dubins_screen_cases()
    out.append(("screens", s, S, G))
    s, S, G, _, _ = M.dubins_curved_cases()
    out.append(("curved", s, S, G))
    for name in ("far_record", "crowd_65"):
        s = M.scene(name)
        out.append((name, s) + M.dubins_edges(s))
    s = M.crowd(129, n_edges=700)
    out.append(("crowd_129", s) + M.dubins_edges(s))
    return out


@pytest.mark.parametrize("column", [_capi.RRTX_TIME_COLUMN_PIECEWISE, _capi.RRTX_TIME_COLUMN_RUNNING_SUM])
def test_dubins_edges_with_time_on_lattice_scenes(oracle, column):
    """dubins_edges_check and dubins_edges_check_obstacle against oracle.dubins_edge_check_polygons_time (batched):
    exact ties of stage 2 and of the chord test at the end node of straight edges, path boxes at R (1 + delta) from the
    edge's box, obstacles 100 from their record centre, lists of 67 and 131 with moving ones at 63, 64, 127, 128.
    The straight edges hold the size of stage 2a's radius and the centre of both boxes; the SIZE of stage 1a's radius
    can drop a hit only on a curved edge: `curved` holds full loops that reach obstacles 3 and 3.5 from the chord's box."""
    piecewise = column == _capi.RRTX_TIME_COLUMN_PIECEWISE
    for name, s, S, G in _dubins_sets():
        assert len(S) <= 1500
        ps = _ps(oracle, s)
        ref = oracle.dubins_edges_batch(S, G, M.R_MIN, ps, s.robot_radius, has_time=True, piecewise=piecewise)
        with Context(4) as ctx:
            _set(ctx, s)
            ctx.set_space_has_time(True)
            ctx.set_dubins_time_column(column)
            cost, word, hit, tl = ctx.dubins_edges_check(S, G, M.R_MIN, s.robot_radius)
            print(f"{name} (column {column}): {len(S)} edges, {int(hit.sum())} hit, {int((hit != ref['hit']).sum())} differ")
            assert np.array_equal(hit, ref["hit"]) and np.array_equal(tl, ref["traj_len"]) and np.array_equal(cost, ref["cost"])
            assert np.array_equal(word, ref["word"])
            for j in _probes(s):
                h = ctx.dubins_edges_check_obstacle(S, G, M.R_MIN, s.robot_radius, j)
                one = oracle.dubins_edges_batch(S, G, M.R_MIN, _one(oracle, s, j), s.robot_radius, has_time=True, piecewise=piecewise)
                assert np.array_equal(h, one["hit"]), (name, j)
        if name not in ("ties", "screens", "curved"):
            assert 0.02 < ref["hit"].mean() < 0.98


# ---- sweeps and releases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dubins", [False, True])
def test_sweeps_of_moving_polygons_on_the_lattice(oracle, dubins):
    """obstacle_sweep_polygon (modes 0 and 1), obstacle_sweep_polygon_batch and obstacle_release_polygon_batch against
    add_new_obstacle_edges / remove_obstacle_edges: nodes exactly at a segment's range, a quarter inside and outside,
    the root exactly at the range of a single query (in by `<=`; its twin, the same place, is out), a one-row and a
    two-row path; the number of candidate edges (stats().last_sweep_candidates) against the oracle's node list, which is
    what sees the one-row path's query.  The plane is [x y t]: a moving polygon is swept there; it is the space WITH time ([x y t theta]) that
    refuses a static one, and a dim = 3 context refuses to be called a space with time."""
    sc = M.sweep_scene(dubins)
    s, pts, es, ee = sc["scene"], sc["pts"], sc["es"], sc["ee"]
    rr, delta, r_min = M.SWEEP_RR, M.SWEEP_DELTA, (M.R_MIN if dubins else 0.0)
    tree = oracle.KDTree(4, wraps=[3], wrap_points=[TWO_PI]) if dubins else oracle.KDTree(3)
    tree.insert_many(pts)
    ps = _ps(oracle, s)
    add = lambda p, j: oracle.add_new_obstacle_edges(tree, pts, es, ee, p, j, rr, delta, dubins, r_min, has_time=True)
    with Context(4 if dubins else 3) as ctx:
        if dubins:
            ctx.set_wrap(3, TWO_PI)
            ctx.set_space_has_time(True)
        else:
            with pytest.raises(RrtxError):
                ctx.set_space_has_time(True)
        ctx.nodes_append(pts)
        _set(ctx, s)
        assert ctx.graph_edges_append(es, ee) == 0
        rows = {}
        for j in s.moving:
            rows[j] = ctx.obstacle_sweep_polygon(j, rr, delta, r_min=r_min, cap=8)
            assert np.array_equal(rows[j], add(ps, j)), j
            # the device's node list itself: every mirrored edge that starts at a node in conflict is a candidate, hit or
            # not -- what holds the one-row path's query and range, whose edges are never hit
            nodes = oracle.points_in_conflict_polygon(tree, ps, j, rr, delta, True, dubins)
            want = int(np.isin(es, nodes).sum())
            assert ctx.stats().last_sweep_candidates == want and want >= len(sc["planted"][j]) // 3, j
        owners = {k: sum(int((es == node).sum() >= 1) for node, name in sc["planted"][3] if name == k) for k in ("at", "in", "out")}
        assert min(owners.values()) >= 6                                 # at / in / out around the one-row path's query
        assert 0 in rows[0] and 1 not in rows[0]                     # edge 0 leaves the root, edge 1 its twin
        assert len(rows[3]) == 0 and sum(len(v) for v in rows.values()) > 60
        if dubins:
            with pytest.raises(RrtxError):                               # a static obstacle in a space with time
                ctx.obstacle_sweep_polygon(4, rr, delta, r_min=r_min)
        else:
            got = ctx.obstacle_sweep_polygon(4, rr, delta)
            assert ctx.stats().last_sweep_candidates == int(np.isin(es, oracle.points_in_conflict_polygon(tree, ps, 4, rr, delta, False, False)).sum())
            assert np.array_equal(got, oracle.add_new_obstacle_edges(tree, pts, es, ee, ps, 4, rr, delta, False)) and len(got) > 0
        order = [3, 1, 0, 2]
        off, ids = ctx.obstacle_sweep_polygon_batch(order, rr, delta, r_min=r_min, cap=8)
        for k, j in enumerate(order):
            assert np.array_equal(ids[off[k]:off[k + 1]], rows[j]), j
        # block what the sweeps found, then the release loops
        blocked = np.zeros(len(es), dtype=bool)
        for j in s.moving:
            blocked[rows[j]] = True
        ctx.graph_edges_block(np.flatnonzero(blocked).astype(np.int32))
        dist = np.where(blocked, np.inf, 1.0)
        freed = 0
        for j in s.moving:
            got = ctx.obstacle_sweep_polygon(j, rr, delta, r_min=r_min, remove=True)
            want = oracle.remove_obstacle_edges(tree, pts, es, ee, dist, ps, j, rr, delta, dubins, r_min, has_time=True)
            assert np.array_equal(got, want), j
            freed += len(got)
        assert freed > 30
        leaving = [2, 0]
        off, ids = ctx.obstacle_release_polygon_batch(leaving, rr, delta, r_min=r_min)
        for k, j in enumerate(leaving):
            act = s.active.copy()
            act[[x for x in leaving if x != j]] = 0
            want = oracle.remove_obstacle_edges(tree, pts, es, ee, dist, _ps(oracle, s, act), j, rr, delta, dubins, r_min, has_time=True)
            assert np.array_equal(ids[off[k]:off[k + 1]], want), j
