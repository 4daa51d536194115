"""RRTX_OPT_DUBINS_TIME_COLUMN = RRTX_TIME_COLUMN_RUNNING_SUM: the time column of a Dubins edge's polyline as the
reference accumulates it (R/DRRT_DubinsEdge_functions.jl:689-695), through every entry point that forms or reads the
stamps, against the oracle's faithful variant (piecewise=False).  Every comparison is ==.  What the scenes must contain
(row counts around the checkpoint spacing, time columns that differ between the two forms, cases whose collision
boolean depends on the form) is asserted on the oracle alone, so no test passes by being empty."""
import json
import math
import os

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from test_gpu_dubins_time import RMIN, RR, VMAX, VMIN, _edges, _env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
PIECEWISE, RUNNING_SUM = _capi.RRTX_TIME_COLUMN_PIECEWISE, _capi.RRTX_TIME_COLUMN_RUNNING_SUM
CKPT = 16                      # kCkptRows of kernels_dubins.hip: the running sum is checkpointed every 16th row
RADII = (1.0, 2.0, 3.0)


def _time_ctx(column):
    ctx = Context(4)
    ctx.set_space_has_time(True)
    ctx.set_dubins_velocity(VMIN, VMAX)
    ctx.set_dubins_time_column(column)
    return ctx


# ---- 1. the option -------------------------------------------------------------------------------------------------
def test_option_plumbing():
    with Context(4) as ctx:
        assert ctx.dubins_time_column == PIECEWISE == 0
        assert ctx.get_option(_capi.RRTX_OPT_DUBINS_TIME_COLUMN) == 0
        ctx.set_dubins_time_column(RUNNING_SUM)
        assert ctx.dubins_time_column == RUNNING_SUM == 1
        for bad in (2, -1):
            with pytest.raises(RrtxError) as ei:
                ctx.set_option(_capi.RRTX_OPT_DUBINS_TIME_COLUMN, bad)
            assert ei.value.code == _capi.RRTX_E_INVALID
            assert ctx.dubins_time_column == RUNNING_SUM
        ctx.set_dubins_time_column(PIECEWISE)
        assert ctx.dubins_time_column == PIECEWISE
    with Context(3) as ctx:                                   # the option exists in every context; only dim = 4 reads it
        ctx.set_dubins_time_column(RUNNING_SUM)
        assert ctx.dubins_time_column == RUNNING_SUM


# ---- 2. trajectory rows ----------------------------------------------------------------------------------------------
def _sweep_edges():
    """Headings and goal offsets swept at three turning radii (no random draws): a general family, goals straight ahead
    with the heading nearly kept (arcs of one or two rows: the shortest polylines) or turned through 0 .. 6.1 rad in
    steps of 0.1 (row counts that grow one by one), the same fine sweep with the goal abeam, and poses shifted sideways
    by 2 .. 3.9 r_min (the three-arc words with three long pieces: the longest polylines the steering gives)."""
    S, G, R = [], [], []

    def add(s, g, r):
        S.append(s); G.append(g); R.append(r)
    for rm in RADII:
        for a in np.arange(2) * math.pi + 0.3:
            for d in (0.0, 0.8, 2.2, 7.0):
                for b in np.arange(3) * (2 * math.pi / 3) + 0.1:
                    for c in np.arange(3) * (2 * math.pi / 3) + 0.9:
                        add([1.0, -2.0, 20.0, a], [1.0 + d * rm * math.cos(b), -2.0 + d * rm * math.sin(b), 17.5,
                                                   (a + c) % (2 * math.pi)], rm)
        for a in (0.0, 3.9):
            for d in (1.5, 5.0):
                for e in (0.0, 0.12, 0.25, 0.45, 1.1, 1.4, 2.9, 3.05, 3.2, 3.3):
                    add([2.0, 1.0, 25.0, a], [2.0 + d * rm * math.cos(a), 1.0 + d * rm * math.sin(a), 22.0, a + e], rm)
        for bo, d in ((0.0, 5.0), (math.pi / 2, 3.0)):
            for e in np.arange(62) * 0.1:
                a = 0.7
                add([2.0, 1.0, 25.0, a], [2.0 + d * rm * math.cos(a + bo), 1.0 + d * rm * math.sin(a + bo), 22.0, a + e], rm)
        for d in np.linspace(2.0, 3.9, 10):
            for e in (-0.02, 0.0, 0.3):
                for sgn in (-1, 1):
                    a = 2.46
                    b = a + sgn * 1.71
                    add([-3.0, 4.0, 30.0, a], [-3.0 + d * rm * math.cos(b), 4.0 + d * rm * math.sin(b), 26.0, a + e], rm)
    return np.array(S), np.array(G), np.array(R)


def test_trajectory_rows_are_the_running_sum(oracle):
    """Row counts P: a polyline is arc + line + arc (at least 1 + 2 + 1 rows) or three arcs, and an arc has at least one
    row, so the steering gives no empty piece and -- as a 2 M-edge random search of the oracle confirms -- no P below 4
    or above 95: P = 2 and P = 3 do not exist, the shortest cases are P = 4 (two one-row arcs around the line), 5 and 6.
    Around every multiple of the checkpoint spacing below the maximum the sweep holds P = 16 c - 1 .. 16 c + 3 (the last
    checkpoint is written at row 16 c <= P - 2 and read by the pieces from row 16 c + 1 on)."""
    S, G, R = _sweep_edges()
    assert 600 <= len(S) <= 1000
    differing = 0
    seen_P, one_row_piece = set(), False
    with _time_ctx(RUNNING_SUM) as ctx:
        for rm in RADII:
            s, g = S[R == rm], G[R == rm]
            ref = oracle.dubins_edges_batch(s, g, rm, has_time=True, piecewise=False, v_min=VMIN, v_max=VMAX, traj=True)
            ref_pw = oracle.dubins_edges_batch(s, g, rm, has_time=True, piecewise=True, v_min=VMIN, v_max=VMAX, traj=True)
            assert np.array_equal(ref["traj"][:, :2], ref_pw["traj"][:, :2])
            differing += int((ref["traj"][:, 2] != ref_pw["traj"][:, 2]).sum())
            seen_P |= set(ref["traj_len"].tolist())
            k = int(np.argmin(ref["traj_len"]))               # the per-edge function gives the same rows as the batch
            assert np.array_equal(oracle.dubins_steer_time(s[k], g[k], rm, piecewise=False)[4],
                                  ref["traj"][ref["traj_off"][k]:ref["traj_off"][k + 1]])
            ctx.set_dubins_time_column(RUNNING_SUM)
            off, traj = ctx.dubins_trajectory(s, g, rm)
            full = ctx.dubins_steer_full(s, g, rm)
            assert np.array_equal(off, ref["traj_off"])
            bad = np.flatnonzero((traj != ref["traj"]).any(axis=1))
            assert bad.size == 0, (rm, int(bad[0]), traj[bad[0]], ref["traj"][bad[0]])
            ctx.set_dubins_time_column(PIECEWISE)
            off0, traj0 = ctx.dubins_trajectory(s, g, rm)
            full0 = ctx.dubins_steer_full(s, g, rm)
            assert np.array_equal(off0, off) and np.array_equal(traj0, ref_pw["traj"])
            for key in ("dist", "wdist", "velocity", "word", "valid_move"):
                assert np.array_equal(full[key], full0[key]), key
            assert np.array_equal(full["dist"], ref["cost"]) and np.array_equal(full["word"], ref["word"])
            # pieces of one row: an edge of 4 rows is two of them around the line
            one_row_piece |= bool((ref["traj_len"] == 4).any())
    want = {4, 5, 6} | {CKPT * c + k for c in range(1, 6) for k in (-1, 0, 1, 2, 3)}
    assert want <= seen_P, sorted(want - seen_P)
    assert max(seen_P) >= 92 and one_row_piece
    assert differing > 1000                                   # the two forms do differ, in thousands of stamps


# ---- 3. edge check, static and moving obstacles ------------------------------------------------------------------------
def test_edges_check_follows_the_running_sum(oracle):
    polys, paths = _env()
    m = len(polys)
    rng = np.random.default_rng(19)
    stat = synth.polygons(24, seed=5)
    all_polys = polys + stat
    kinds = [6 if i % 2 else 7 for i in range(m)] + [3] * len(stat)
    all_paths = paths + [None] * len(stat)
    active = np.ones(len(all_polys), dtype=np.uint8)
    active[[2, m + 3]] = 0
    ps = oracle.PolygonSet(all_polys, kinds=kinds, paths=all_paths, active=active)
    s, g = _edges(rng, 2500, spread=20.0)
    t_hi = max(p[:, 2].max() for p in paths)
    s[:, 2] = rng.uniform(0.0, t_hi, len(s)); g[:, 2] = s[:, 2] - rng.uniform(0.05, 6.0, len(s))
    ref = oracle.dubins_edges_batch(s, g, RMIN, has_time=True, piecewise=False, traj=True)
    off, rows = ref["traj_off"], ref["traj"]
    want = np.array([oracle.dubins_edge_check_polygons_time(ps, s[k], g[k], rows[off[k]:off[k + 1]], RR, RMIN)[0]
                     for k in range(len(s))])
    assert 0.05 < want.mean() < 0.9
    with _time_ctx(PIECEWISE) as ctx:
        ctx.polygons_set(all_polys, kinds=kinds, paths=all_paths, active=active)
        cost0, word0, hit0, tl0 = ctx.dubins_edges_check(s, g, RMIN, RR)
        ctx.set_dubins_time_column(RUNNING_SUM)
        cost, word, hit, tl = ctx.dubins_edges_check(s, g, RMIN, RR)
        assert np.array_equal(hit.astype(bool), want), np.flatnonzero(hit.astype(bool) != want)[:8]
        assert np.array_equal(cost, cost0) and np.array_equal(word, word0) and np.array_equal(tl, tl0)
        assert np.array_equal(cost, ref["cost"]) and np.array_equal(tl, ref["traj_len"])
        # one obstacle alone: a moving one, a static one, an inactive one (list positions)
        for j in (1, m + 5, 2):
            h = ctx.dubins_edges_check_obstacle(s, g, RMIN, RR, j)
            one = oracle.PolygonSet([all_polys[j]], kinds=[kinds[j]], paths=[all_paths[j]], active=[active[j]])
            w1 = np.array([oracle.dubins_edge_check_polygons_time(one, s[k], g[k], rows[off[k]:off[k + 1]], RR, RMIN)[0]
                           for k in range(len(s))])
            assert np.array_equal(h.astype(bool), w1), (j, np.flatnonzero(h.astype(bool) != w1)[:8])
            assert w1.any() == bool(active[j])


# ---- 4. cases whose boolean depends on the form -------------------------------------------------------------------------
def test_check_kernel_sides_with_the_selected_form(oracle):
    """tests/golden/time_column_flips.json (tests/make_time_column_flips.py, an oracle-only search): edges with a moving
    obstacle that grazes one deep piece of a long arc, where the two time columns give different collision booleans.
    A check kernel that ignored the option would fail half of these under one of its values."""
    d = json.load(open(os.path.join(ROOT, "golden", "time_column_flips.json")))
    cases, rr = d["cases"], d["robot_radius"]
    assert len(cases) >= 16
    assert any(c["hit_running_sum"] for c in cases) and any(c["hit_piecewise"] for c in cases)
    with _time_ctx(PIECEWISE) as ctx:
        for n, c in enumerate(cases):
            s, g, rm = np.array(c["s"]), np.array(c["g"]), c["r_min"]
            poly, path = np.array(c["polygon"]), np.array(c["path"])
            ps = oracle.PolygonSet([poly], kinds=[6], paths=[path])
            tr_rs = oracle.dubins_steer_time(s, g, rm, piecewise=False)[4]
            tr_pw = oracle.dubins_steer_time(s, g, rm, piecewise=True)[4]
            h_rs = oracle.dubins_edge_check_polygons_time(ps, s, g, tr_rs, rr, rm)[0]
            h_pw = oracle.dubins_edge_check_polygons_time(ps, s, g, tr_pw, rr, rm)[0]
            assert (h_rs, h_pw) == (c["hit_running_sum"], c["hit_piecewise"]) and h_rs != h_pw, n
            assert c["row"] >= 20 and len(tr_rs) == c["rows"]
            ctx.polygons_set([poly], kinds=[6], paths=[path])
            ctx.set_dubins_time_column(RUNNING_SUM)
            got_rs = bool(ctx.dubins_edges_check(s[None], g[None], rm, rr)[2][0])
            ctx.set_dubins_time_column(PIECEWISE)
            got_pw = bool(ctx.dubins_edges_check(s[None], g[None], rm, rr)[2][0])
            assert (got_rs, got_pw) == (h_rs, h_pw), (n, got_rs, got_pw, h_rs, h_pw)


# ---- 5. the fused preamble ------------------------------------------------------------------------------------------------
def _preamble_scene(oracle):
    polys, paths = _env()
    kinds = [6] * len(polys)
    rng = np.random.default_rng(23)
    n, nq = 6000, 40
    pts = synth.nodes(n, 4)
    pts[:, 2] = rng.uniform(10.0, 35.0, n)
    Q = synth.queries(nq, 4)
    Q[:, 2] = rng.uniform(10.0, 35.0, nq)
    return polys, paths, kinds, pts, Q


def _preamble_ctx(polys, paths, kinds, pts, column):
    ctx = _time_ctx(column)
    ctx.set_wrap(3, 2.0 * math.pi)
    ctx.nodes_append(pts)
    ctx.polygons_set(polys, kinds=kinds, paths=paths)
    return ctx


def test_fused_preamble_follows_the_running_sum(oracle):
    polys, paths, kinds, pts, Q = _preamble_scene(oracle)
    ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths)
    r = 9.0
    with _preamble_ctx(polys, paths, kinds, pts, PIECEWISE) as ctx:
        out0 = ctx.extend_candidates_dubins(Q, r, RR, RMIN)
        ctx.set_dubins_time_column(RUNNING_SUM)
        out = ctx.extend_candidates_dubins(Q, r, RR, RMIN)
    assert len(out["idx"]) > 200
    for k in ("offsets", "idx", "key"):
        assert np.array_equal(out[k], out0[k]), k
    ref = oracle.dubins_candidates_batch(Q, out["offsets"], out["idx"], pts, RMIN, ps, RR, has_time=True, piecewise=False,
                                         v_min=VMIN, v_max=VMAX)
    for k in ("cost_out", "cost_in", "hit_out", "hit_in"):
        bad = np.flatnonzero(out[k] != ref[k])
        assert bad.size == 0, (k, int(bad[0]), out[k][bad[0]], ref[k][bad[0]])
    both = out["hit_out"].astype(int) | out["hit_in"].astype(int)
    assert (both & 2).any() and (out["hit_out"] & 1).any()


# ---- 6. the two composed paths ----------------------------------------------------------------------------------------------
def test_find_new_target_uses_the_same_edges(oracle):
    """Under the running sum, every adopted target is what the fused preamble's own flags and costs select around that
    pose at radius_used: the two share the steering, checkpoint and check launches."""
    polys, paths, kinds, pts, Q = _preamble_scene(oracle)
    poses = Q[:32]
    rng = np.random.default_rng(29)
    lmc = rng.uniform(0.0, 50.0, len(pts))
    with _preamble_ctx(polys, paths, kinds, pts, RUNNING_SUM) as ctx:
        out = ctx.find_new_target_dubins(poses, 4.0, 40.0, RR, RMIN, lmc=lmc)
        ok = out["status"] == _capi.RRTX_TGT_OK
        assert ok.sum() >= 16
        for i in np.flatnonzero(ok):
            ec = ctx.extend_candidates_dubins(poses[i:i + 1], float(out["radius_used"][i]), RR, RMIN)
            free = ec["hit_out"] == 0
            cand = np.where(free, lmc[ec["idx"]] + ec["cost_out"], np.inf)
            e = int(np.argmin(cand))                          # (the first of equal minima)
            assert np.isfinite(cand[e]) and ec["idx"][e] == out["target_idx"][i], i
            assert ec["hit_out"][e] == 0 and out["edge_dist"][i] == ec["cost_out"][e] and out["cost_to_goal"][i] == cand[e], i


def test_obstacle_sweep_returns_what_the_edge_check_flags(oracle):
    env = json.load(open(os.path.join(ROOT, "golden", "env_inputs.json")))
    mv = [np.array(p) for p in env["rand_StaticTime_7_polygons"]][:6]
    mv_paths = [np.array(p) for p in env["rand_StaticTime_7_paths"]][:6]
    kinds = [6, 7, 6, 7, 6, 7]
    rng = np.random.default_rng(31)
    n = 1200
    pts = np.c_[rng.uniform(-30.0, 30.0, (n, 2)), rng.uniform(0.0, 30.0, n), rng.uniform(0, 2 * math.pi, n)]
    d2 = ((pts[:, None, :2] - pts[None, :, :2]) ** 2).sum(axis=2)
    es, ee = np.nonzero((d2 < 5.5 ** 2) & (pts[:, None, 2] > pts[None, :, 2]))    # start later than end (reverse time)
    es, ee = es.astype(np.int32), ee.astype(np.int32)
    assert 15000 < len(es) < 25000
    tree = oracle.KDTree(4, wraps=[3], wrap_points=[2.0 * math.pi])
    tree.insert_many(pts)
    ps = oracle.PolygonSet(mv, kinds=kinds, paths=mv_paths)
    r_min, delta = synth.R_MIN_TIME, 8.0
    with _time_ctx(RUNNING_SUM) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(mv, kinds=kinds, paths=mv_paths)
        ctx.graph_edges_append(es, ee)
        total = 0
        for j in (0, 3):
            got = ctx.obstacle_sweep_polygon(j, RR, delta, r_min=r_min)
            nodes = oracle.points_in_conflict_polygon(tree, ps, j, RR, delta, True, True)
            cand = np.flatnonzero(np.isin(es, nodes))
            assert len(cand) > 100
            h = ctx.dubins_edges_check_obstacle(pts[es[cand]], pts[ee[cand]], r_min, RR, j)
            assert np.array_equal(got, cand[h != 0]), j
            total += len(got)
        assert total > 20
