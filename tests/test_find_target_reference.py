"""The reference for findNewTarget (R/DRRT_Q.jl:2901-2994) that the device tests compare against, built only from what
oracle/oracle.py exports, in two forms that are held against each other here:

  find_target_loop   the literal per-pose loop: kdFindWithinRange at r0, then kdFindMoreWithinRange at 2 r0, 4 r0, ...
                     (KDTree.within_range(r0, q, more=[...]), the oracle's own accumulation), the returned set walked in
                     ascending node index with one steer and one edge check per neighbour;
  find_target_batch  the same from range_batch (per-pose radii) + candidates_batch / dubins_candidates_batch and a
                     first minimum per segment.  A later round searches the whole ball again: what lay inside the
                     previous ball was rejected by a deterministic test, so the answer is the same.

Both return the six outputs of rrtx_find_new_target; every comparison is np.array_equal.  These tests pass with and
without the device feature: they pin the reference."""
import json
import math
import os

import numpy as np
import pytest

KEYS = ("target_idx", "edge_dist", "cost_to_goal", "radius_used", "rounds", "status")
TGT_OK, TGT_NOT_FOUND = 0, 1
ROOT = os.path.dirname(os.path.abspath(__file__))


class Scene:
    """What both forms need to know: the edge type, the obstacle list and the steering parameters."""

    def __init__(self, kind, nodes, obs, robot_radius, r_min=0.0, v_min=0.0, v_max=0.0, wraps=None, wrap_points=None):
        assert kind in ("spheres", "polygons", "dubins", "dubins_time")
        self.kind, self.obs, self.rr, self.r_min, self.v_min, self.v_max = kind, obs, robot_radius, r_min, v_min, v_max
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        self.d = self.nodes.shape[1]
        self.wraps, self.wrap_points = wraps, wrap_points

    def tree(self, O):
        t = O.KDTree(self.d, self.wraps, self.wrap_points)
        t.insert_many(self.nodes)
        return t

    def tree_set(self, O):
        return O.TreeSet(self.d, self.nodes, wraps=self.wraps, wrap_points=self.wrap_points)

    def edge(self, O, a, b):
        """(edge.dist, blocked) of the directed edge a -> b, one edge at a time"""
        if self.kind == "spheres":
            return O.euclid(a, b), O.edge_check_spheres(self.obs[0], self.obs[1], a, b, self.rr)[0]
        if self.kind == "polygons":
            return O.euclid(a, b), O.edge_check_polygons(self.obs, a, b, self.rr)[0]
        if self.kind == "dubins":
            cost, _, traj = O.dubins_steer(a, b, self.r_min)
            return cost, O.dubins_edge_check_polygons(self.obs, a, b, traj, self.rr, self.r_min)[0]
        dist, _, vel, _, traj = O.dubins_steer_time(a, b, self.r_min, piecewise=True)
        hit = O.dubins_edge_check_polygons_time(self.obs, a, b, traj, self.rr, self.r_min)[0]
        return dist, hit or not O.dubins_valid_move_time(a, b, vel, self.v_min, self.v_max)

    def edges(self, O, Q, offsets, idx):
        """(edge.dist, blocked byte) of pose -> node for every CSR entry, batched"""
        if self.kind in ("spheres", "polygons"):
            c = O.candidates_batch(Q, offsets, idx, self.nodes, self.obs, self.rr)
        else:
            t = self.kind == "dubins_time"
            c = O.dubins_candidates_batch(Q, offsets, idx, self.nodes, self.r_min, self.obs, self.rr, has_time=t,
                                          piecewise=t, v_min=self.v_min, v_max=self.v_max)
        return c["cost_out"], c["hit_out"]


def _empty(nq):
    return dict(target_idx=np.full(nq, -1, dtype=np.int32), edge_dist=np.full(nq, math.inf),
                cost_to_goal=np.full(nq, math.inf), radius_used=np.zeros(nq), rounds=np.zeros(nq, dtype=np.int32),
                status=np.full(nq, TGT_NOT_FOUND, dtype=np.uint8))


def differs_from_nearest_safe(ref):
    """Share of the OK poses whose target is not the nearest node they could have taken (find_target_batch only)"""
    ok = ref["status"] == TGT_OK
    return float((ref["target_idx"][ok] != ref["nearest_safe"][ok]).mean()) if ok.any() else 0.0


def find_target_loop(O, scene, tree, poses, r0, r_max, lmc):
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, scene.d)
    nq = len(poses)
    r0 = np.broadcast_to(np.asarray(r0, dtype=np.float64), (nq,))
    out = _empty(nq)
    for i in range(nq):
        r, k, more = float(r0[i]), 1, []
        while True:
            idx, _ = tree.within_range(float(r0[i]), poses[i], more=more)
            assert len(np.unique(idx)) == len(idx)
            best, winner, winner_cost = math.inf, -1, math.inf
            for j in np.sort(idx):
                cost, blocked = scene.edge(O, poses[i], scene.nodes[j])
                cand = lmc[j] + cost
                if not blocked and cand < best:
                    best, winner, winner_cost = cand, int(j), cost
            if best != math.inf:
                out["status"][i], out["target_idx"][i], out["edge_dist"][i] = TGT_OK, winner, winner_cost
                out["cost_to_goal"][i], out["radius_used"][i], out["rounds"][i] = best, r, k
                break
            last = r
            r = r * 2
            if r > r_max:
                out["radius_used"][i], out["rounds"][i] = last, k
                break
            more.append((r, poses[i]))
            k += 1
    return out


def find_target_batch(O, scene, trees, poses, r0, r_max, lmc, stats=None):
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, scene.d)
    nq = len(poses)
    r = np.array(np.broadcast_to(np.asarray(r0, dtype=np.float64), (nq,)))
    lmc = np.asarray(lmc, dtype=np.float64)
    out = _empty(nq)
    out["nearest_safe"] = np.full(nq, -1, dtype=np.int32)      # (not an output of the call: a property of the scene)
    act = np.arange(nq)
    k = 1
    while act.size:
        Q = np.ascontiguousarray(poses[act])
        rng = O.range_batch(trees, Q, r[act] if act.size > 1 else float(r[act][0]), nearest=False)
        off, idx = rng["offsets"], rng["idx"]
        cost, hit = scene.edges(O, Q, off, idx)
        with np.errstate(invalid="ignore"):
            cand = lmc[idx] + cost
        ok = (hit == 0) & (cand < math.inf)            # (a NaN compares false)
        masked = np.where(ok, cand, math.inf)
        if stats is not None:
            stats.append(dict(poses=int(act.size), entries=int(len(idx))))
        go_on = []
        for a, i in enumerate(act):
            seg = masked[off[a]:off[a + 1]]
            j = int(np.argmin(seg)) if seg.size else -1        # argmin: the first of equal minima
            if j >= 0 and seg[j] < math.inf:
                e = off[a] + j
                out["status"][i], out["target_idx"][i], out["edge_dist"][i] = TGT_OK, idx[e], cost[e]
                out["cost_to_goal"][i], out["radius_used"][i], out["rounds"][i] = cand[e], r[i], k
                out["nearest_safe"][i] = idx[off[a] + int(np.argmin(np.where(ok[off[a]:off[a + 1]], cost[off[a]:off[a + 1]], math.inf)))]
                continue
            if r[i] * 2 > r_max:
                out["radius_used"][i], out["rounds"][i] = r[i], k
                continue
            r[i] = r[i] * 2
            go_on.append(i)
        act = np.array(go_on, dtype=np.int64)
        k += 1
    return out


def lmc_for_rounds(O, trees, nodes, poses, r0, seed, nan_count=16):
    """rrtLMC that makes rounds necessary by construction: uniform values, the root at 0, a few NaN, and for pose i every
    node within r0[i] * 2^(j_i - 1) * 0.99 set to +Inf with j_i cycling through 0, 1, 2, 3 -- the ball of round j_i
    (radius r0 * 2^(j_i - 1)) then holds orphans only, bar a thin shell, and round j_i + 1 is the first that can
    answer.  Returns (lmc, j)."""
    n, nq = len(nodes), len(poses)
    rng = np.random.default_rng(seed)
    lmc = rng.uniform(0.0, 60.0, n)
    lmc[rng.integers(1, n, nan_count)] = math.nan
    j = np.arange(nq) % 4
    blocked = O.range_batch(trees, poses, np.asarray(r0, dtype=np.float64) * 2.0 ** (j - 1) * 0.99, nearest=False)
    lmc[blocked["idx"]] = math.inf
    lmc[0] = 0.0
    return lmc, j


def c4_scene(nq, seed, polygons=False):
    """The C4 tree (N = 200 k, 256 spheres, or 64 polygons) with nq poses: the configuration's samples, some next to
    obstacle centres, some far outside the world, r0 drawn per pose over a factor of 8.
    Returns (pts, obstacles as the context takes them, poses, r0, r_max)."""
    from rrtqx_3d_amd import synth
    cfg = synth.CONFIGS["C4"]
    pts = synth.nodes(cfg.n_nodes, 3)
    rng = np.random.default_rng(seed)
    poses = synth.queries(nq, 3, seed=seed + 1).copy()
    if polygons:
        obs = synth.polygons(64)
        centres = np.array([np.concatenate([p.mean(axis=0), [0.0]]) for p in obs])
    else:
        obs = synth.spheres(cfg.n_obstacles)
        centres = obs[:, :3]
    k = nq // 16
    poses[:k] = centres[np.arange(k) % len(centres)] + rng.uniform(-0.4, 0.4, (k, 3))
    if polygons:
        poses[:k, 2] = rng.uniform(-synth.WORLD, synth.WORLD, k)
    far = rng.uniform(-1.0, 1.0, (k, 3))
    poses[k:2 * k] = far / np.linalg.norm(far, axis=1)[:, None] * rng.uniform(90.0, 400.0, (k, 1))
    r0 = 0.4 * 8.0 ** rng.random(nq)
    return pts, obs, poses, r0, 24.0


def _assert_same(a, b, what=""):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k)


def _random_lmc(rng, n):
    lmc = rng.uniform(0.0, 60.0, n)
    lmc[rng.random(n) < 0.3] = math.inf
    lmc[rng.integers(1, n, 8)] = math.nan
    lmc[0] = 0.0
    return lmc


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_loop_equals_batch_simple_edge(oracle, kind):
    from rrtqx_3d_amd import synth
    O = oracle
    n, nq = 4000, 96
    rng = np.random.default_rng(31)
    pts = synth.nodes(n, 3)
    obs = O.make_spheres(synth.spheres(48)) if kind == "spheres" else O.PolygonSet(synth.polygons(24))
    scene = Scene(kind, pts, obs, 0.5)
    poses = synth.queries(nq, 3, seed=77).copy()
    poses[:6] = (synth.spheres(48)[:6, :3] if kind == "spheres" else
                 np.array([np.concatenate([p.mean(axis=0), [3.0]]) for p in synth.polygons(24)[:6]])) + 0.125
    poses[6:10] = np.array([300.0, -200.0, 150.0]) + np.arange(4)[:, None]
    r0 = 1.5 * 8.0 ** rng.random(nq)
    ts = scene.tree_set(O)
    lmc, _ = lmc_for_rounds(O, ts, pts, poses, r0, seed=5)
    r_max = 60.0
    stats = []
    ref = find_target_batch(O, scene, ts, poses, r0, r_max, lmc, stats)
    _assert_same(find_target_loop(O, scene, scene.tree(O), poses, r0, r_max, lmc), ref, kind)
    assert {TGT_OK, TGT_NOT_FOUND} == set(ref["status"].tolist())
    assert len(set(ref["rounds"].tolist())) >= 3 and len(stats) >= 3
    ok = ref["status"] == TGT_OK
    assert np.array_equal(ref["cost_to_goal"][ok], lmc[ref["target_idx"][ok]] + ref["edge_dist"][ok])
    assert (ref["target_idx"][~ok] == -1).all() and np.isinf(ref["cost_to_goal"][~ok]).all()
    assert (ref["radius_used"][~ok] * 2 > r_max).all()
    # a scalar first radius is the same as that radius for every pose
    _assert_same(find_target_batch(O, scene, ts, poses, 3.0, r_max, lmc),
                 find_target_batch(O, scene, ts, poses, np.full(nq, 3.0), r_max, lmc), "scalar r0")


def test_root_exactly_at_the_range(oracle):
    """The root is taken with <=, every other node with <: a pose exactly r0 from both finds the root in round 1 and the
    other node only once the ball has doubled."""
    O = oracle
    pts = np.array([[10.0, 10.0, 10.0], [18.0, 10.0, 10.0], [40.0, 40.0, 40.0]])
    scene = Scene("spheres", pts, O.make_spheres(np.array([[-40.0, -40.0, -40.0, 1.0]])), 0.5)
    pose = np.array([[14.0, 10.0, 10.0]])
    ts = scene.tree_set(O)
    for lmc, want in (([0.0, 1.0, 1.0], (0, 4.0, 4.0, 4.0, 1)), ([math.inf, 1.0, 1.0], (1, 4.0, 5.0, 8.0, 2))):
        ref = find_target_batch(O, scene, ts, pose, 4.0, 100.0, np.array(lmc))
        _assert_same(find_target_loop(O, scene, scene.tree(O), pose, 4.0, 100.0, np.array(lmc)), ref)
        got = tuple(ref[k][0] for k in ("target_idx", "edge_dist", "cost_to_goal", "radius_used", "rounds"))
        assert got == want and ref["status"][0] == TGT_OK


def dubins_scene(O, has_time, n, nq, seed):
    """A Dubins tree with theta wrapped: static polygons, or the moving ones of rand_StaticTime_7 in a space with time.
    Returns (scene, context polygons dict, poses, r0, r_max)."""
    from rrtqx_3d_amd import synth
    rng = np.random.default_rng(seed)
    if has_time:
        env = json.load(open(os.path.join(ROOT, "golden", "env_inputs.json")))
        polys = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_polygons"]][::-1]
        paths = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_paths"]][::-1]
        kinds = [6] * len(polys)
        pts, poses = synth.nodes(n, 4), synth.queries(nq, 4, seed=seed + 1)
        pts[:, 2] = rng.uniform(10.0, 30.0, n)
        poses[:, 2] = rng.uniform(20.0, 35.0, nq)          # (planning runs in reverse time: the pose is later than its target)
        ps = O.PolygonSet(polys, kinds=kinds, paths=paths)
        scene = Scene("dubins_time", pts, ps, 0.5, r_min=2.0, v_min=5.0, v_max=30.0, wraps=[3], wrap_points=[2.0 * math.pi])
        ctx_polys = dict(polys=polys, kinds=kinds, paths=paths)
    else:
        polys = synth.polygons(24)
        pts, poses = synth.nodes(n, 4), synth.queries(nq, 4, seed=seed + 1)
        scene = Scene("dubins", pts, O.PolygonSet(polys), 0.5, r_min=1.0, wraps=[3], wrap_points=[2.0 * math.pi])
        ctx_polys = dict(polys=polys)
    poses[: nq // 4, 3] = rng.choice([0.02, 2.0 * math.pi - 0.02], nq // 4)      # next to the wrap: ghosts matter
    r0 = 3.0 * 2.0 ** rng.random(nq)
    return scene, ctx_polys, poses, r0, 40.0


@pytest.mark.parametrize("has_time", [False, True])
def test_loop_equals_batch_dubins_wrapped_theta(oracle, has_time):
    O = oracle
    scene, _, poses, r0, r_max = dubins_scene(O, has_time, 3000, 24, seed=11)
    ts = scene.tree_set(O)
    lmc, _ = lmc_for_rounds(O, ts, scene.nodes, poses, r0 * 2.0, seed=6)
    ref = find_target_batch(O, scene, ts, poses, r0, r_max, lmc)
    _assert_same(find_target_loop(O, scene, scene.tree(O), poses, r0, r_max, lmc), ref, has_time)
    assert (ref["rounds"] >= 2).sum() >= 2 and (ref["status"] == TGT_OK).sum() >= 4
    # the wrap matters: the lists of the poses next to theta = 0 / 2 pi hold nodes that only a ghost reaches
    flat = Scene(scene.kind, scene.nodes, scene.obs, scene.rr, scene.r_min, scene.v_min, scene.v_max)
    with_ghosts = O.range_batch(ts, poses, 12.0, nearest=False)
    without = O.range_batch(flat.tree_set(O), poses, 12.0, nearest=False)
    assert with_ghosts["offsets"][-1] > without["offsets"][-1] > 0
