"""The lattice tori of tests/torus_model.py: the oracle's wrapped searches (up to three wraps, both wrap orders) held
to the plain numpy restatement of the ghost rule bit for bit, and the scenes held to the boundary cases that
tests/test_gpu_torus.py relies on.  No GPU.

The counts: 16 of every case the GPU test relies on, in every scene; the root cases are planted, one query each.  A
count that depends on the radius (all copies searched, ghosts on the skip threshold) is asked of the per-query radius
array and of at least one scalar radius.

T3 / T3r cannot differ in a key: two copies that shift different dimensions both reach a node only when
sqrt(p_a^2 + p_b^2) < 2 r, which periods of 8 and 4 exclude for r < 4, and a copy always precedes the same copy with one
more dimension shifted, in either order.  That is asserted, and the order of the wraps is tested on T3s / T3sr (periods
4, 4, 8), whose keys do differ.

Two of the rules decide nothing while every node lies inside [0, period] (torus_model.side_scene says why): the side a
query at exactly period / 2 is shifted to, and whether a ghost exactly on the skip threshold is searched.  The side
scenes, with nodes just below 0, are held here to the cases that make them decide."""
import functools

import numpy as np
import pytest

import torus_model as M

SCENES = sorted(M.SPACES)


def _radii(sc):
    return [(str(r), r) for r in sc["radii"]] + [("mix", sc["r_mix"])]


@functools.lru_cache(maxsize=None)
def _cases(name):
    sc = M.scene(name)
    return {label: M.cases(sc["nodes"], sc["Q"], r, sc["wraps"], sc["periods"]) for label, r in _radii(sc)}


@functools.lru_cache(maxsize=None)
def _tree(name):
    from oracle import oracle as O
    sc = M.scene(name)
    t = O.KDTree(sc["dim"], list(sc["wraps"]), list(sc["periods"]))
    t.insert_many(sc["nodes"])
    return t


@pytest.mark.parametrize("name", SCENES)
def test_scene_is_a_lattice_inside_its_periods(name):
    sc = M.scene(name)
    nodes, Q = sc["nodes"], sc["Q"]
    assert len(np.unique(nodes, axis=0)) == len(nodes)
    for d in range(sc["dim"]):
        per = dict(zip(sc["wraps"], sc["periods"])).get(d)
        for P in (nodes, Q):
            if per == M.TWO_PI:
                assert set(P[:, d].tolist()) <= {k * (np.pi / 4) for k in range(9)}
                assert 0.0 in P[:, d] and M.TWO_PI in P[:, d]
            else:
                assert np.array_equal(P[:, d] * 4.0, np.round(P[:, d] * 4.0))
            if per is not None:                 # the nearest search is the minimum over all copies only then
                assert P[:, d].min() >= 0.0 and P[:, d].max() <= per
    assert set(np.unique(sc["r_mix"]).tolist()) == set(M.RADII)


@pytest.mark.parametrize("name", SCENES)
def test_oracle_range_search_equals_the_restatement(oracle, name):
    sc = M.scene(name)
    tree = _tree(name)
    total = 0
    for label, r in _radii(sc):
        ref = M.range_lists(sc["nodes"], sc["Q"], r, sc["wraps"], sc["periods"])
        rq = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(sc["Q"]),))
        for i, q in enumerate(sc["Q"]):
            oi, ok = tree.within_range(float(rq[i]), q)
            o = np.argsort(oi, kind="stable")
            a, b = ref["offsets"][i], ref["offsets"][i + 1]
            assert np.array_equal(oi[o], ref["idx"][a:b]), f"{name} r={label} query {i}: sets differ"
            assert np.array_equal(ok[o].view(np.uint64), ref["key"][a:b].view(np.uint64)), f"{name} r={label} query {i}: keys differ"
        # the batched form the GPU tests compare against is the same search
        rb = oracle.range_batch(tree, sc["Q"], r, nearest=False)
        assert np.array_equal(rb["offsets"], ref["offsets"]) and np.array_equal(rb["idx"], ref["idx"])
        assert np.array_equal(rb["key"].view(np.uint64), ref["key"].view(np.uint64))
        total += len(ref["idx"])
    print(f"{name}: {total} neighbours")


@pytest.mark.parametrize("name", SCENES)
def test_oracle_nearest_and_ghost_iterator_equal_the_restatement(oracle, name):
    sc = M.scene(name)
    tree = _tree(name)
    want = M.nearest(sc["nodes"], sc["Q"], sc["wraps"], sc["periods"])
    got_i, got_d = zip(*(tree.nearest(q) for q in sc["Q"]))
    assert np.array_equal(np.array(got_d).view(np.uint64), want.view(np.uint64))
    # on nodes inside [0, period] that is the minimum over every copy, skipped or not
    G, _ = M.copies(sc["Q"], sc["wraps"], sc["periods"])
    every = np.sqrt(M.sq(G[:, :, None, :], sc["nodes"][None, None])).min(axis=(0, 2))
    assert np.array_equal(want, every)
    assert (M.copy_dists(sc["nodes"][list(got_i)], sc["Q"], sc["wraps"], sc["periods"]) == want[None]).any(axis=0).all()
    for r in sc["radii"]:
        v = M.searched(sc["Q"], r, sc["wraps"], sc["periods"])
        for i, q in enumerate(sc["Q"]):
            g = tree.ghost_points(q, r)
            assert np.array_equal(g, G[1:, i][v[1:, i]]), f"{name} r={r} query {i}: ghosts differ"


@pytest.mark.parametrize("name", SCENES)
def test_scene_holds_the_boundary_cases(name):
    sc = M.scene(name)
    c = _cases(name)
    for label, v in c.items():
        print(name, label, v)
    scalar = [c[str(r)] for r in sc["radii"]]
    for k in ("all_copies", "on_skip"):
        assert c["mix"][k] >= 16 and max(x[k] for x in scalar) >= 16, k
    for x in scalar + [c["mix"]]:
        assert x["at_r_unlisted"] >= 16
    shortest = min(sc["periods"])
    for r, x in zip(sc["radii"], scalar):
        if r > shortest / 2.0:
            assert x["multi_seen"] >= 16 and x["key_not_min"] >= 16, r
        else:
            assert x["multi_seen"] == 0
    assert c["mix"]["multi_seen"] >= 16 and c["mix"]["key_not_min"] >= 16
    for k in ("at_half", "at_zero", "at_period"):
        assert c["mix"][k] >= 16, k
    # the planted root cases, at every radius and in the mixed array (query i of radius i keeps its own radius)
    for x in scalar:
        assert x["root_at_r_listed"] >= 1 and x["root_at_r_ghost"] >= 1
    assert c["mix"]["root_at_r_listed"] >= len(sc["radii"]) and c["mix"]["root_at_r_ghost"] >= len(sc["radii"])
    # the root exactly at r from a ghost that is searched before the copy that lists it: wherever a period of 4 meets
    # r > 2 on the lattice (theta of D4 is no lattice)
    if name != "D4":
        assert c["mix"]["root_at_r_then_later"] >= 1 and max(x["root_at_r_then_later"] for x in scalar) >= 1


def _lists(name, r):
    sc = M.scene(name)
    return M.range_lists(sc["nodes"], sc["Q"], r, sc["wraps"], sc["periods"])


def test_wrap_order_changes_keys_where_two_short_periods_meet():
    for a, b in (("T3", "T3r"), ("T3s", "T3sr")):
        assert np.array_equal(M.scene(a)["nodes"], M.scene(b)["nodes"]) and np.array_equal(M.scene(a)["Q"], M.scene(b)["Q"])
        assert sorted(M.scene(a)["wraps"]) == sorted(M.scene(b)["wraps"]) and M.scene(a)["wraps"] != M.scene(b)["wraps"]
        assert dict(zip(M.scene(a)["wraps"], M.scene(a)["periods"])) == dict(zip(M.scene(b)["wraps"], M.scene(b)["periods"]))
    differ = 0
    for r in M.RADII:
        la, lb = _lists("T3", r), _lists("T3r", r)
        for k in ("offsets", "idx", "key"):                     # periods 8, 4, 8: the order renumbers copies, no more
            assert np.array_equal(la[k], lb[k])
        assert not np.array_equal(la["slot"], lb["slot"])
        sa, sb = _lists("T3s", r), _lists("T3sr", r)
        assert np.array_equal(sa["offsets"], sb["offsets"]) and np.array_equal(sa["idx"], sb["idx"])
        differ += int((sa["key"] != sb["key"]).sum())
    print(f"T3s / T3sr: {differ} keys differ")
    assert differ >= 16


def _side_tree(oracle, sc):
    t = oracle.KDTree(sc["dim"], list(sc["wraps"]), list(sc["periods"]))
    t.insert_many(sc["nodes"])
    return t


@pytest.mark.parametrize("axis", [0, 1])
def test_side_scenes_make_the_side_test_and_the_skip_threshold_decide(oracle, axis):
    sc = M.side_scene(axis)
    nodes, Q, wraps, periods = sc["nodes"], sc["Q"], sc["wraps"], sc["periods"]
    assert (nodes[:, axis] < 0.0).all() and np.array_equal(nodes * 4.0, np.round(nodes * 4.0))
    half = Q[:, axis] == periods[axis] / 2.0
    assert half.sum() >= 32
    tree = _side_tree(oracle, sc)
    G, Cl = M.copies(Q, wraps, periods)
    # nearest: the oracle equals the restatement, which here is still the minimum over every copy, and every query at
    # period / 2 is answered by a shifted copy -- the one the strict < picks
    want = M.nearest(nodes, Q, wraps, periods)
    assert np.array_equal(np.array([tree.nearest(q)[1] for q in Q]), want)
    per_copy = np.sqrt(M.sq(G[:, :, None, :], nodes[None, None])).min(axis=2)
    assert np.array_equal(want, per_copy.min(axis=0))
    assert (per_copy[0][half] > want[half]).all()
    up = Q.copy()
    up[half, axis] += periods[axis]                               # where <= would send the copy
    assert (np.sqrt(M.sq(up[:, None, :], nodes[None])).min(axis=1)[half] > want[half]).all()
    by_ghost = on_threshold = 0
    for label, r in _radii(sc):
        ref = M.range_lists(nodes, Q, r, wraps, periods)
        rb = oracle.range_batch(tree, Q, r, nearest=False)
        assert np.array_equal(rb["offsets"], ref["offsets"]) and np.array_equal(rb["idx"], ref["idx"])
        assert np.array_equal(rb["key"].view(np.uint64), ref["key"].view(np.uint64))
        owner = np.repeat(np.arange(len(Q)), np.diff(ref["offsets"]))
        by_ghost += int(((ref["slot"] > 0) & half[owner]).sum())
        on_skip = np.sqrt(M.sq(Cl, G)) == np.broadcast_to(np.asarray(r, dtype=np.float64), (len(Q),))[None]
        on_threshold += int(on_skip[ref["slot"], owner].sum())
    print(f"side {axis}: {by_ghost} entries by the ghost of a query at period / 2, {on_threshold} by a ghost on the skip threshold")
    if axis == 0:
        assert on_threshold >= 16          # (a query at 4 = 8 / 2 has its ghost 4 > r away from the period: never searched)
    else:
        assert by_ghost >= 16


def test_planar_torus_of_the_sweeps(oracle):
    sc = M.planar_scene()
    nodes, es, ee = sc["nodes"], sc["es"], sc["ee"]
    assert (nodes[:, 2] == 0.0).all() and len(np.unique(nodes, axis=0)) == len(nodes)
    assert nodes[:, 0].max() <= 8.0 and nodes[:, 1].max() <= 4.0 and nodes.min() >= 0.0
    ps = oracle.PolygonSet(sc["polys"])
    tree = oracle.KDTree(3, list(sc["wraps"]), list(sc["periods"]))
    tree.insert_many(nodes)
    on_range = last_copy = 0
    for j, (c, r) in enumerate(zip(sc["centres"], sc["ranges"])):
        assert (ps.arr[j].cx, ps.arr[j].cy) == (c[0], c[1]) and float(r) in M.RADII
        assert r == M.SWEEP_RR + M.SWEEP_DELTA + ps.arr[j].radius
        q = np.array([[c[0], c[1], 0.0]])
        lists = M.range_lists(nodes, q, float(r), sc["wraps"], sc["periods"])
        got = np.sort(oracle.points_in_conflict_polygon(tree, ps, j, M.SWEEP_RR, M.SWEEP_DELTA, False, False))
        assert np.array_equal(got, lists["idx"])
        slot = np.full(len(nodes), -1)
        slot[lists["idx"]] = lists["slot"]
        want = oracle.add_new_obstacle_edges(tree, nodes, es, ee, ps, j, M.SWEEP_RR, M.SWEEP_DELTA, dubins=False)
        last_copy += int((slot[es[want]] == 3).sum())
        dist, _ = M.reach(nodes, q, float(r), sc["wraps"], sc["periods"])
        on_range += int(((dist[1:, 0] == r) & M.searched(q, float(r), sc["wraps"], sc["periods"])[1:]).sum())
    print(f"planar torus: {last_copy} edges through the last copy, {on_range} nodes on a ghost's range")
    assert last_copy >= 16 and on_range >= 16
