"""findNewTarget on the device (rrtx_find_new_target, rrtx_find_new_target_dubins, drrt.findNewTarget) against
find_target_batch of tests/test_find_target_reference.py (which that file holds against the literal per-pose loop).
Every comparison is np.array_equal on all six outputs: each is an input value, an index, one rounded fp64 addition or
r0 * 2^j.  What the scenes must contain -- every number of rounds, both statuses, targets that are not the nearest safe
node, exact ties -- is asserted on the reference alone, so no test passes by being empty."""
import ctypes as C
import math

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, drrt, synth
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from test_find_target_reference import (KEYS, TGT_NOT_FOUND, TGT_OK, Scene, c4_scene, differs_from_nearest_safe,
                                        dubins_scene, find_target_batch, find_target_loop, lmc_for_rounds)

pytestmark = pytest.mark.gpu
RR = 0.5
C4_SEED = 41


def _assert_same(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype, (what, k, got[k].dtype, ref[k].dtype)
        bad = np.flatnonzero(~((got[k] == ref[k]) | ((got[k] != got[k]) & (ref[k] != ref[k]))))
        assert bad.size == 0, (what, k, int(bad[0]), {n: (got[n][bad[0]], ref[n][bad[0]]) for n in KEYS})
        assert np.array_equal(got[k], ref[k]), (what, k)


# ---- C4 size -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obstacles,nq", [("spheres", 4096), ("polygons", 1024)])
def test_c4_tree(oracle, obstacles, nq):
    O = oracle
    poly = obstacles == "polygons"
    pts, obs, poses, r0, r_max = c4_scene(nq, C4_SEED, polygons=poly)
    scene = Scene(obstacles, pts, O.PolygonSet(obs) if poly else O.make_spheres(obs), RR)
    ts = scene.tree_set(O)
    lmc, _ = lmc_for_rounds(O, ts, pts, poses, r0, seed=C4_SEED + 2)
    assert lmc[0] == 0.0 and np.isnan(lmc).any() and np.isinf(lmc).any()
    stats = []
    ref = find_target_batch(O, scene, ts, poses, r0, r_max, lmc, stats)
    # the scene, judged on the reference alone
    share = np.bincount(ref["rounds"], minlength=5) / nq
    print("rounds share", share, "per round", stats, "not nearest", differs_from_nearest_safe(ref))
    assert (share[1:5] >= 0.05).all(), share
    assert {TGT_OK, TGT_NOT_FOUND} == set(ref["status"].tolist())
    assert differs_from_nearest_safe(ref) >= 0.10
    assert r0.max() / r0.min() > 6.0
    with Context(3, node_capacity=len(pts)) as ctx:
        ctx.nodes_append(pts)
        if poly:
            ctx.polygons_set(obs)
            ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        else:
            ctx.spheres_set(obs)
        got = ctx.find_new_target(poses, r0, r_max, RR, lmc=lmc)
        _assert_same(got, ref, obstacles)
        settled = ctx.get_option(_capi.RRTX_OPT_SELECT_LIST_CAP)
        assert settled >= max(s["entries"] for s in stats)
        _assert_same(ctx.find_new_target(poses, r0, r_max, RR, lmc=lmc), ref, "again")
        # lmc = NULL: the context's own array, uploaded in two parts (NaN and Inf travel as they are)
        n = len(pts)
        ctx.node_cost_set(0, lmc[:n // 3])
        ctx.node_cost_set(n // 3, lmc[n // 3:])
        _assert_same(ctx.find_new_target(poses, r0, r_max, RR), ref, "node_cost_set")
        # capacity growth: a round that overflows the lists is run again with room, the results are unchanged
        ctx.set_option(_capi.RRTX_OPT_SELECT_LIST_CAP, 64)
        _assert_same(ctx.find_new_target(poses, r0, r_max, RR, lmc=lmc), ref, "grown")
        assert ctx.get_option(_capi.RRTX_OPT_SELECT_LIST_CAP) >= max(s["entries"] for s in stats)
        # the four agents of the reference's driver, one first radius for all
        four = find_target_batch(O, scene, ts, poses[-4:], 3.0, r_max, lmc)
        _assert_same(ctx.find_new_target(poses[-4:], 3.0, r_max, RR, lmc=lmc), four, "four agents")
        # the other entry points still answer as before after the lists were used by this one
        lists = ctx.extend_candidates(poses[:64], 3.0, RR)
        want = O.range_batch(ts, poses[:64], 3.0, nearest=False)
        assert np.array_equal(lists["offsets"], want["offsets"]) and np.array_equal(lists["idx"], want["idx"])


# ---- exact ties ------------------------------------------------------------------------------------------------------
def test_lattice_ties_go_to_the_lowest_index(oracle):
    O = oracle
    rng = np.random.default_rng(3)
    P = np.unique(rng.integers(0, 64, (20000, 3)) / 4.0, axis=0)
    P = P[rng.permutation(len(P))]
    poses = rng.integers(0, 64, (2048, 3)) / 4.0
    lmc = rng.integers(0, 12, len(P)) / 4.0
    lmc[rng.random(len(P)) < 0.5] = math.inf
    lmc[0] = 0.0
    sph = np.concatenate([rng.integers(8, 56, (6, 3)) / 4.0, np.full((6, 1), 1.5)], axis=1)
    scene = Scene("spheres", P, O.make_spheres(sph), RR)
    ts = scene.tree_set(O)
    r0 = np.where(np.arange(len(poses)) % 2 == 0, 0.5, 1.0)
    ref = find_target_batch(O, scene, ts, poses, r0, 4.0, lmc)
    # ties in the reference: poses whose winning value is offered by a second, higher-indexed safe neighbour
    ok = np.flatnonzero(ref["status"] == TGT_OK)
    lists = O.range_batch(ts, poses[ok], ref["radius_used"][ok], nearest=False)
    c = O.candidates_batch(poses[ok], lists["offsets"], lists["idx"], P, scene.obs, RR)
    cand = np.where(c["hit_out"] == 0, lmc[lists["idx"]] + c["cost_out"], math.inf)
    owner = np.repeat(np.arange(len(ok)), np.diff(lists["offsets"]))
    at_best = cand == ref["cost_to_goal"][ok][owner]
    ties = np.bincount(owner[at_best], minlength=len(ok))
    assert (ties >= 2).sum() >= 16
    first = lists["idx"][np.array([np.flatnonzero((owner == a) & at_best)[0] for a in np.flatnonzero(ties >= 2)])]
    assert np.array_equal(first, ref["target_idx"][ok][ties >= 2])             # the lowest index, since lists ascend
    assert len(set(ref["rounds"].tolist())) >= 2
    with Context(3) as ctx:
        ctx.nodes_append(P)
        ctx.spheres_set(sph)
        _assert_same(ctx.find_new_target(poses, r0, 4.0, RR, lmc=lmc), ref, "lattice")


# ---- NOT_FOUND and the limits ----------------------------------------------------------------------------------------
def test_not_found_and_limits(oracle):
    O = oracle
    n = 6000
    pts = synth.nodes(n, 3)
    sph = synth.spheres(16)
    scene = Scene("spheres", pts, O.make_spheres(sph), RR)
    ts = scene.tree_set(O)
    poses = synth.queries(50, 3, seed=9)
    lmc = np.random.default_rng(4).uniform(0.0, 50.0, n)
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        # every node an orphan: the ball doubles to the limit and nothing is found
        inf = np.full(n, math.inf)
        ref = find_target_batch(O, scene, ts, poses, 5.0, 60.0, inf)
        assert (ref["status"] == TGT_NOT_FOUND).all() and (ref["rounds"] == 4).all() and (ref["radius_used"] == 40.0).all()
        _assert_same(ctx.find_new_target(poses, 5.0, 60.0, RR, lmc=inf), ref, "all orphans")
        # r_max < 2 r0: one round, whatever it finds
        ref = find_target_batch(O, scene, ts, poses, 5.0, 9.0, lmc)
        assert (ref["rounds"] == 1).all() and {TGT_OK, TGT_NOT_FOUND} >= set(ref["status"].tolist())
        _assert_same(ctx.find_new_target(poses, 5.0, 9.0, RR, lmc=lmc), ref, "one round")
        ref = find_target_batch(O, scene, ts, poses, 12.0, 9.0, lmc)            # (the first search is always at r0)
        assert (ref["rounds"] == 1).all() and (ref["status"] == TGT_OK).all()
        _assert_same(ctx.find_new_target(poses, 12.0, 9.0, RR, lmc=lmc), ref, "r0 beyond r_max")
        # every edge blocked: the pose sits at the centre of a sphere (distancePointToSegment is 0 for every edge from there)
        inside = sph[:8, :3].copy()
        ref = find_target_batch(O, scene, ts, inside, 6.0, 100.0, lmc)
        assert (ref["status"] == TGT_NOT_FOUND).all() and (ref["rounds"] == 5).all()
        _assert_same(ctx.find_new_target(inside, 6.0, 100.0, RR, lmc=lmc), ref, "inside a sphere")
        # nq = 0
        e = ctx.find_new_target(np.zeros((0, 3)), 5.0, 60.0, RR, lmc=lmc)
        assert all(len(e[k]) == 0 for k in KEYS)
        # bad radii
        for r0, r_max in ((0.0, 60.0), (-1.0, 60.0), (math.nan, 60.0), (math.inf, 60.0), (5.0, math.inf), (5.0, math.nan),
                          (60.0 * 2.0 ** -41, 60.0)):
            with pytest.raises(RrtxError) as err:
                ctx.find_new_target(poses, r0, r_max, RR, lmc=lmc)
            assert err.value.code == _capi.RRTX_E_INVALID, (r0, r_max)
        bad = np.full(50, 5.0); bad[37] = 0.0
        with pytest.raises(RrtxError) as err:
            ctx.find_new_target(poses, bad, 60.0, RR, lmc=lmc)
        assert err.value.code == _capi.RRTX_E_INVALID
        ok = ctx.find_new_target(poses[:2], 60.0 * 2.0 ** -40, 60.0, RR, lmc=lmc)      # the smallest radius accepted
        _assert_same(ok, find_target_batch(O, scene, ts, poses[:2], 60.0 * 2.0 ** -40, 60.0, lmc), "41 rounds at most")
        # wrong edge type for the context
        with pytest.raises(RrtxError) as err:
            ctx.find_new_target_dubins(np.zeros((1, 3)), 5.0, 60.0, RR, 1.0, lmc=lmc)
        assert err.value.code == _capi.RRTX_E_STATE
    with Context(4) as ctx4:
        ctx4.nodes_append(synth.nodes(64, 4))
        with pytest.raises(RrtxError) as err:
            ctx4.find_new_target(synth.queries(4, 4), 5.0, 60.0, RR, lmc=np.zeros(64))
        assert err.value.code == _capi.RRTX_E_STATE
    with Context(3) as empty:
        with pytest.raises(RrtxError) as err:
            empty.find_new_target(poses, 5.0, 60.0, RR)
        assert err.value.code == _capi.RRTX_E_STATE
    with Context(3) as wrapped:
        wrapped.set_wrap(2, 2.0 * math.pi)
        wrapped.nodes_append(pts)
        with pytest.raises(RrtxError) as err:
            wrapped.find_new_target(poses, 5.0, 60.0, RR, lmc=lmc)
        assert err.value.code == _capi.RRTX_E_STATE


def test_1025_poses_that_all_need_a_second_round(oracle):
    """The poses that go on are compacted by ONE workgroup of 1024: 1025 of them take two passes of its loop, in every
    round.  First with orphans only within r0 of every pose (all go on after round 1, most find a target later),
    then with every node an orphan (all 1025 go on in every round and end NOT_FOUND)."""
    O = oracle
    n, nq = 6000, 1025
    pts = synth.nodes(n, 3)
    sph = synth.spheres(16)
    scene = Scene("spheres", pts, O.make_spheres(sph), RR)
    ts = scene.tree_set(O)
    poses = synth.queries(nq, 3, seed=10)
    r0 = np.full(nq, 5.0)
    lmc = np.random.default_rng(6).uniform(0.0, 50.0, n)
    lmc[O.range_batch(ts, poses, r0, nearest=False)["idx"]] = math.inf
    ref = find_target_batch(O, scene, ts, poses, r0, 60.0, lmc)
    print("rounds", np.bincount(ref["rounds"]), "ok", (ref["status"] == TGT_OK).sum())
    assert (ref["rounds"] >= 2).all() and (ref["status"] == TGT_OK).sum() > nq // 2
    inf = np.full(n, math.inf)
    ref_inf = find_target_batch(O, scene, ts, poses, r0, 60.0, inf)
    assert (ref_inf["status"] == TGT_NOT_FOUND).all() and (ref_inf["rounds"] == 4).all()
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        _assert_same(ctx.find_new_target(poses, r0, 60.0, RR, lmc=lmc), ref, "second round")
        _assert_same(ctx.find_new_target(poses, r0, 60.0, RR, lmc=inf), ref_inf, "all orphans")


# ---- Dubins ----------------------------------------------------------------------------------------------------------
def _lmc_second_round(O, ts, n, poses, r0, seed):
    """Every second pose has only orphans within 0.99 r0: it needs the second round."""
    rng = np.random.default_rng(seed)
    lmc = rng.uniform(0.0, 80.0, n)
    lmc[rng.random(n) < 0.1] = math.inf
    sel = np.arange(1, len(poses), 2)
    lmc[O.range_batch(ts, poses[sel], r0[sel] * 0.99, nearest=False)["idx"]] = math.inf
    lmc[0] = 0.0
    return lmc


def test_dubins_c3_tree(oracle):
    O = oracle
    cfg = synth.CONFIGS["C3"]
    pts, polys = synth.nodes(cfg.n_nodes, 4), synth.polygons(cfg.n_obstacles)
    nq, r_min, r_max = 64, 1.0, 30.0
    rng = np.random.default_rng(12)
    poses = synth.queries(nq, 4, seed=88).copy()
    poses[:16, 3] = rng.choice([0.02, 2.0 * math.pi - 0.02], 16)               # next to the wrap
    r0 = 2.5 * 2.0 ** rng.random(nq)
    scene = Scene("dubins", pts, O.PolygonSet(polys), RR, r_min=r_min, wraps=[3], wrap_points=[2.0 * math.pi])
    ts = scene.tree_set(O)
    lmc = _lmc_second_round(O, ts, len(pts), poses, r0, seed=13)
    ref = find_target_batch(O, scene, ts, poses, r0, r_max, lmc)
    print("rounds", np.bincount(ref["rounds"]), "ok", (ref["status"] == TGT_OK).sum())
    assert (ref["rounds"] >= 2).sum() >= 2 and (ref["status"] == TGT_OK).sum() >= nq // 2
    with Context(4, node_capacity=len(pts)) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys)
        _assert_same(ctx.find_new_target_dubins(poses, r0, r_max, RR, r_min, lmc=lmc), ref, "C3")
        ctx.node_cost_set(0, lmc)
        _assert_same(ctx.find_new_target_dubins(poses, r0, r_max, RR, r_min), ref, "C3, node_cost_set")


def test_dubins_with_time(oracle):
    O = oracle
    scene, cp, poses, r0, r_max = dubins_scene(O, True, 6000, 32, seed=11)
    ts = scene.tree_set(O)
    lmc = _lmc_second_round(O, ts, len(scene.nodes), poses, r0, seed=14)
    ref = find_target_batch(O, scene, ts, poses, r0, r_max, lmc)
    print("rounds", np.bincount(ref["rounds"]), "ok", (ref["status"] == TGT_OK).sum())
    assert (ref["rounds"] >= 2).sum() >= 2 and (ref["status"] == TGT_OK).sum() >= 8
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(scene.nodes)
        ctx.polygons_set(cp["polys"], kinds=cp["kinds"], paths=cp["paths"])
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(scene.v_min, scene.v_max)
        _assert_same(ctx.find_new_target_dubins(poses, r0, r_max, RR, scene.r_min, lmc=lmc), ref, "time")


# ---- the reference-named call ----------------------------------------------------------------------------------------
def test_drrt_find_new_target_on_the_planner_scene(oracle):
    from test_gpu_planner_loop import HI, LO, ROBOT_RADIUS, _spheres
    O = oracle
    sph = _spheres()
    rng = np.random.default_rng(21)
    n = 3000
    pts = rng.uniform(LO, HI, (n, 3))
    KD = drrt.KDTree(3)
    S = drrt.CSpace(3, 0.0, [LO] * 3, [HI] * 3, [0, 0, 0], [0, 0, 0])
    S.robotRadius = ROBOT_RADIUS
    S.bind(KD)
    for row in sph[::-1]:
        drrt.addObsToCSpace(S, drrt.SphereObstacle(row))
    nodes = [drrt.RRTNode(p) for p in pts]
    drrt.kdInsertMany(KD, nodes)
    lmc = rng.uniform(0.0, 40.0, n)
    lmc[rng.random(n) < 0.6] = math.inf
    lmc[0] = 0.0
    robot_poses = rng.uniform(LO, HI, (4, 3))
    old = [nodes[int(k)] for k in rng.integers(0, n, 4)]
    hyper = 1.5
    r_max = O.euclid(S.lowerBounds, S.upperBounds)
    r0 = np.array([min(max(hyper, O.euclid(p, t.position)), r_max) for p, t in zip(robot_poses, old)])
    scene = Scene("spheres", pts, O.make_spheres(sph), ROBOT_RADIUS)
    ref = find_target_loop(O, scene, scene.tree(O), robot_poses, r0, r_max, lmc)
    assert (ref["status"] == TGT_OK).all()
    robots = [drrt.RobotData(p, t) for p, t in zip(robot_poses, old)]
    out = drrt.findNewTarget(S, KD, robots, hyper, lmc=lmc)
    _assert_same(out, ref, "drrt")
    for i, R in enumerate(robots):
        assert R.nextMoveTarget is nodes[ref["target_idx"][i]] and R.currentMoveInvalid is False
        assert R.distanceFromNextRobotPoseToNextMoveTarget == ref["edge_dist"][i]
    # one robot, rrtLMC from the context's own array
    KD.ctx.node_cost_set(0, lmc)
    one = drrt.RobotData(robot_poses[2], old[2])
    drrt.findNewTarget(S, KD, one, hyper)
    assert one.nextMoveTarget is nodes[ref["target_idx"][2]]
    # it raises where the reference does
    far = drrt.RobotData([4000.0, 4000.0, 4000.0], nodes[0])
    far.nextMoveTarget = None
    with pytest.raises(RuntimeError, match="unable to find a valid move target"):
        drrt.findNewTarget(S, KD, far, hyper, lmc=lmc)
    with pytest.raises(RuntimeError, match="unable to find a valid move target"):
        drrt.findNewTarget(S, KD, drrt.RobotData(robot_poses[0], old[0]), hyper, lmc=np.full(n, math.inf))
    assert C.sizeof(C.c_double) == 8
