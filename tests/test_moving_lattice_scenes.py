"""The lattice-in-time scenes of tests/moving_lattice_model.py, judged without a device: the model (a numpy restatement
of the moving branch of explicitEdgeCheck2D) agrees with the oracle on every edge of every scene, first-hit index
included, and each scene holds what it was built for -- exact ties in every clamp state, edge times on row times,
every kind of NaN quotient, obstacles far from their record centre, crowded lists.  The counts are printed and
asserted.  tests/test_gpu_moving_lattice.py runs the same scenes through the C-ABI.

The hand-worked answers at the end pin the oracle itself on the four decisions no uniform scene reaches; they follow
from the rule as DESIGN.md 4.6 and the oracle's comments state it, not from running the oracle."""
import numpy as np
import pytest

import moving_lattice_model as M

ALL = list(M.SCENES)


@pytest.fixture(scope="module")
def stat(oracle):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = M.static_hits(oracle, M.scene(name))
        return memo[name]
    return get


@pytest.mark.parametrize("name", ALL)
def test_model_agrees_with_the_oracle(oracle, stat, name):
    s = M.scene(name)
    ps = s.polygon_set(oracle)
    hit, first = M.list_check(s, stat(name))
    ohit, ofirst = oracle.edges_check_batch(ps, s.p0, s.p1, s.robot_radius)
    assert np.array_equal(hit, ohit) and np.array_equal(first, ofirst)
    # one obstacle alone, for every moving one (the active flag is the list's business)
    for j in s.moving[:40]:
        one = oracle.PolygonSet([s.polys[j]], kinds=[s.kinds[j]], paths=[s.paths[j]])
        assert np.array_equal(M.obstacle_hits(s, j), oracle.edges_check_batch(one, s.p0, s.p1, s.robot_radius)[0].astype(bool)), j
    rate = float(hit.mean())
    print(f"{name}: {len(s.p0)} edges, {s.m} obstacles ({len(s.moving)} moving), hit rate {rate:.3f}")
    if name != "nan":
        assert 0.05 <= rate <= 0.95


@pytest.mark.parametrize("name", ALL)
def test_model_points_agree_with_the_oracle(oracle, name):
    """findTransformObsToTimeOfPoint: flag and clearance of the moving branch equal the static branch's on diamonds
    moved by the model's offset -- at row times, before the first row, after the last, at clearance exactly 0"""
    s = M.scene(name)
    ps = s.polygon_set(oracle)
    pts = M.scene_points(s)[:600]
    unsafe, clr = M.points_expected(oracle, s, pts)
    ounsafe, oclr = oracle.points_check_batch(ps, pts, s.robot_radius)
    assert np.array_equal(unsafe, ounsafe) and np.array_equal(clr, oclr)
    zero = int(((clr == 0.0) & (unsafe == 0)).sum())
    print(f"{name}: {len(pts)} points, {int(unsafe.sum())} unsafe, {zero} safe at clearance exactly 0")
    assert 0 < unsafe.sum() < len(pts)
    if name in ("knots", "far_record", "lattice_random") or name.startswith("tangent"):
        assert zero >= 5


@pytest.mark.parametrize("name", ["tangent_0.25", "tangent_0.5", "tangent_1"])
def test_tangent_holds_exact_ties_in_every_clamp_state(name):
    s = M.scene(name)
    tests, ties = M.count_states(s)
    print(f"{name}: segment tests lo/in/hi/nan {tests.tolist()}, exact ties {ties.tolist()}")
    assert ties[M.LO] >= 20 and ties[M.IN] >= 20 and ties[M.HI] >= 20
    for tag in ("in", "in_lo", "in_hi", "lo", "hi"):
        _, t = M.count_states(s, tag)
        k = {"in": M.IN, "in_lo": M.IN, "in_hi": M.IN, "lo": M.LO, "hi": M.HI}[tag]
        print(f"  built as {tag}: {len(s.tags[tag])} edges, ties {t.tolist()}")
        assert t[k] >= 20                                   # in_lo / in_hi: T_c exactly ON a clamp, still `in`
    # a tie is no hit under `<` and a hit under `<=`; one lattice step to a side decides either way
    hit, _ = M.list_check(s)
    le, _ = M.list_check(s, le_final=True)
    built = np.concatenate([s.tags[t] for t in ("in", "in_lo", "in_hi", "lo", "hi")])
    near = np.concatenate([s.tags["near_" + t] for t in ("in", "in_lo", "in_hi", "lo", "hi")])
    print(f"  ties: {int(hit[built].sum())} of {len(built)} hit; with <= {int(le[built].sum())}; one step aside {hit[near].mean():.3f} hit")
    assert (le[built] & ~hit[built]).sum() >= 100
    assert 0.2 < hit[near].mean() < 0.8


def test_knots_hold_edge_times_on_row_times():
    s = M.scene("knots")
    hit, _ = M.list_check(s)
    le, _ = M.list_check(s, le_index=True)
    for tag in ("first", "inner", "last"):
        e = s.tags[tag]
        on = np.zeros(len(e), dtype=bool)
        for j in s.moving:
            rows = s.paths[j][:, 2]
            pick = {"first": rows[:1], "inner": rows[1:-1], "last": rows[-1:]}[tag]
            on |= np.isin(s.p0[e, 2], pick) | np.isin(s.p1[e, 2], pick)
        print(f"knots: {int(on.sum())} edges with a time on a {tag} row time, {int(hit[e].sum())} hit, "
              f"{int((hit[e] != le[e]).sum())} change under <= in findIndexBeforeTime")
        assert on.sum() >= 20 and 0 < hit[e].sum() < len(e)
    assert (hit[s.tags["first"]] != le[s.tags["first"]]).sum() >= 20
    assert (hit[s.tags["last"]] != le[s.tags["last"]]).sum() >= 20
    # wholly before / after the path: never tested, whatever lies on top of what
    for tag in ("before", "after"):
        assert len(s.tags[tag]) >= 20 and not hit[s.tags[tag]].any()
    fwd = s.p0[:, 2] < s.p1[:, 2]
    assert 0.3 < fwd.mean() < 0.7 and hit[fwd].any() and hit[~fwd].any()      # both time directions


def test_nan_scene_holds_every_nan_kind_and_none_hits(oracle):
    s = M.scene("nan")
    ps = s.polygon_set(oracle)
    ohit, _ = oracle.edges_check_batch(ps, s.p0, s.p1, s.robot_radius)
    for tag in ("same_velocity", "zero_duration", "zero_length", "repeat_mid", "repeat_end", "single_row"):
        e = s.tags[tag]
        nan_tests = 0
        for j in s.moving:
            t = M.segment_tests(*s.centres[j], s.radii[j], s.paths[j], s.p0[e], s.p1[e], s.robot_radius)
            if tag.startswith("repeat"):
                twin = np.diff(s.paths[j][:, 2]) == 0
                k = t["tested"][:, twin] & np.isnan(t["margin"][:, twin])
            else:
                k = t["tested"] & np.isnan(t["margin"])
            nan_tests += int(k.sum())
            assert not (t["tested"] & (t["state"] == M.NAN) & (t["margin"] < 0)).any()
        print(f"nan: {tag}: {len(e)} edges, {nan_tests} NaN segment tests, {int(ohit[e].sum())} edges hit")
        assert len(e) >= 20
        if tag == "single_row":      # the one-row path is never tested (NaN tests counted here are a far twin-row obstacle's)
            one = [j for j in s.moving if len(s.paths[j]) == 1]
            assert len(one) == 1 and not ohit[e].any()
            assert np.hypot(*(s.p0[e, :2] - (np.array(s.centres[one[0]]) + s.paths[one[0]][0, :2])).T).min() == 0.0
        else:
            assert nan_tests >= 20
        if tag in ("same_velocity", "zero_duration", "zero_length"):
            assert not ohit[e].any()                                     # the NaN test is the only one these edges get
    # the twin-row edges do meet ordinary segments beside the NaN one: some hit, some do not
    e = np.concatenate([s.tags["repeat_mid"], s.tags["repeat_end"]])
    assert 0 < ohit[e].sum() < len(e)
    assert ohit[s.tags["rest_vs_moving"]].any()                          # a robot at rest is an ordinary test


def test_far_record_hits_far_from_every_record_centre(oracle):
    s = M.scene("far_record")
    ps = s.polygon_set(oracle)
    ohit, _ = oracle.edges_check_batch(ps, s.p0, s.p1, s.robot_radius)
    nearest = np.inf
    for j in range(s.m):
        c = np.array(s.centres[j])
        d = np.minimum(np.hypot(*(s.p0[:, :2] - c).T), np.hypot(*(s.p1[:, :2] - c).T)) - np.hypot(*(s.p1[:, :2] - s.p0[:, :2]).T)
        nearest = min(nearest, float(d.min()) - (s.radii[j] + s.robot_radius))
        carried = c + s.paths[j][:, :2]
        assert np.hypot(*(carried - c).T).min() >= 100.0
    print(f"far_record: hit rate {ohit.mean():.3f}; no edge within {nearest:.1f} of a record centre's inflated circle")
    assert ohit.mean() >= 0.20 and nearest > 100.0


@pytest.mark.parametrize("m", [33, 65, 257])
def test_crowd_list_positions(m):
    s = M.scene("crowd_%d" % m)
    assert s.m == m + 2 and int(s.active.sum()) == m and {3, 6, 7} <= set(s.kinds)
    for pos in M.CROWD_MOVING_AT:
        if pos < s.m:
            assert s.kinds[pos] in (6, 7) and s.active[pos]
    assert sum(1 for j in range(32) if s.kinds[j] in (6, 7) and s.active[j]) >= 5       # 64 edges x 5: the queue of 256 flushes


def test_lattice_random_breadth():
    s = M.scene("lattice_random")
    tests, ties = M.count_states(s)
    print(f"lattice_random: {int(tests.sum())} segment tests, lo/in/hi/nan {tests.tolist()}, exact ties {ties.tolist()}")
    assert len(s.p0) == 4000 and s.m == 24 and tests.sum() > 20_000 and (tests[:3] > 1000).all()


# ---- hand-worked known answers (beside M1 .. M3 of tests/test_oracle_kat.py) -----------------------------------------
def test_hand_worked_known_answers(oracle):
    """Obstacle: diamond of radius 1 about the origin (centre (0, 0), bounding radius 1), path rows (dx, dy, t) =
    (0, 0, 0), (4, 0, 4), (4, 4, 8): along +x at speed 1, then along +y at speed 1.  Robot radius 1/4: rr = 5/4.

    M4  an edge time equal to a row time.  Robot (4, 1, t=8) -> (20, 1, t=9) starts ON the last row's time, 1 from where
        the obstacle ends, (4, 4).  findIndexBeforeTime(8) counts rows with t < 8 strictly: 2, so firstObsInd = 2;
        findIndexBeforeTime(9) = 3, lastObsInd = min(4, 3) = 3: segment 2 is tested.  m1 = (16, 0), m2 = (0, 1),
        T_c = (256 * 8 + 0 - 0 + (0 - 1) * (0 - 4 - 1 + 0)) / (256 + 1) = 2053 / 257 < 8 = max(T_1, T_2): clamped to 8
        (also the upper clamp, min(9, 8)); robot at (4, 1), obstacle at (4, 4): 9 > 25/16, no hit.  With the robot at
        (4, 3.25): 9/16 < 25/16, HIT -- a `<=` in findIndexBeforeTime would give firstObsInd = lastObsInd = 3 and test
        nothing.  A quarter later (t = 8.25 -> 9.25) the edge lies after the path: 3, min(4, 3) = 3, nothing tested.
        The end on the FIRST row's time: (20, 0, t=-1) -> (0.5, 0, t=0): findIndexBeforeTime(0) = 0, lastObsInd = 1 <=
        firstObsInd = 1: no test, although the robot ends inside the obstacle.
    M5  the tie at rr^2.  Robot (2.75, 1, t=1) -> (2.75, 1, t=3) rests at (2.75, 1) while the obstacle passes along
        y = 0: m1 = 0, m2 = (1, 0), T_c = (0 + 1 * (0 + 2.75 - 0) - 0) / 1 =
        2.75, inside [1, 3]; obstacle at (2.75, 0): d^2 = 1 < 25/16: hit.  At (2, 1.25): T_c = 2, d^2 = 25/16: NOT a hit
        (`<`), a quarter nearer, (2, 1): hit.  The 3-4-5 tie in the `lo` state: (2.75, 1, t=2) -> (5.75, 5, t=3):
        m1 = (3, 4), relative velocity (2, 4), offset at t = 2 (0.75, 1): moving apart, T_c < 2 is clamped to 2,
        d^2 = 9/16 + 1 = 25/16 exactly: no hit; from (2.5, 1): d^2 = 1/4 + 1 < 25/16: hit.
    M6  equal velocities.  Robot (0.5, 0.5, t=0) -> (2.5, 0.5, t=2) rides along with the obstacle, inside it: m1 = m2,
        num = 0, den = 0, T_c = NaN, every comparison false: no hit.  One quarter faster in y it is an ordinary hit.
    M7  a single-row path.  firstObsInd = max(.., 1) = 1, lastObsInd = min(.., 1) = 1: never tested."""
    D = M.diamond(0.0, 0.0, 1.0)
    ps = oracle.PolygonSet([D], kinds=[6], paths=[[[0, 0, 0], [4, 0, 4], [4, 4, 8]]])
    assert ps.centre_radius().tolist() == [[0.0, 0.0, 1.0]]
    chk = lambda a, b: int(oracle.edges_check_polygons(ps, np.array([a], float), np.array([b], float), 0.25)[0][0])
    # M4
    assert chk([4, 1, 8], [20, 1, 9]) == 0
    assert chk([4, 3.25, 8], [20, 3.25, 9]) == 1 and chk([20, 3.25, 9], [4, 3.25, 8]) == 1
    assert chk([4, 3.25, 8.25], [20, 3.25, 9.25]) == 0
    assert chk([20, 0, -1], [0.5, 0, 0]) == 0 and chk([20, 0, -0.75], [0.5, 0, 0.25]) == 1
    # M5
    assert chk([2.75, 1, 1], [2.75, 1, 3]) == 1
    assert chk([2, 1.25, 1], [2, 1.25, 3]) == 0 and chk([2, 1, 1], [2, 1, 3]) == 1
    assert chk([2.75, 1, 2], [5.75, 5, 3]) == 0 and chk([2.5, 1, 2], [5.5, 5, 3]) == 1
    # M6
    assert chk([0.5, 0.5, 0], [2.5, 0.5, 2]) == 0 and chk([0.5, 0.5, 0], [2.5, 1.0, 2]) == 1
    # M7
    one = oracle.PolygonSet([D], kinds=[7], paths=[[[0, 0, 5]]])
    for a, b in (([0, 0, 4], [0.25, 0, 6]), ([0, 0, 5], [0.25, 0, 6]), ([0, 0, 4], [0.25, 0, 5]), ([0, 0, 5], [0, 0, 5])):
        assert not oracle.edge_check_polygons(one, a, b, 0.25)[0]
    # the model restates the same rule: the same answers, and the states named above
    t = M.segment_tests(0.0, 0.0, 1.0, ps.paths[0], np.array([[2, 1.25, 1], [2.75, 1, 2], [0.5, 0.5, 0], [4, 3.25, 8.0]]),
                        np.array([[2, 1.25, 3], [5.75, 5, 3], [2.5, 0.5, 2], [20, 3.25, 9.0]]), 0.25)
    assert t["tested"].tolist() == [[True, False], [True, False], [True, False], [False, True]]
    assert [t["state"][0, 0], t["state"][1, 0], t["state"][2, 0], t["state"][3, 1]] == [M.IN, M.LO, M.NAN, M.LO]
    assert t["T_c"][0, 0] == 2.0 and t["margin"][0, 0] == 0.0 and t["margin"][1, 0] == 0.0 and t["margin"][3, 1] < 0


# ---- the Dubins and sweep scenes of tests/test_gpu_moving_lattice.py ---------------------------------------------------
@pytest.mark.parametrize("piecewise", [True, False])
def test_dubins_ties_are_ties_for_the_oracle(oracle, piecewise):
    s, S, G, tags = M.dubins_ties()
    ps = s.polygon_set(oracle)
    r = oracle.dubins_edges_batch(S, G, M.R_MIN, ps, s.robot_radius, has_time=True, piecewise=piecewise)
    assert (r["traj_len"] == 4).all()                        # straight: two arcs of one row each and the line
    n = {t: (int(r["hit"][tags == t].sum()), int((tags == t).sum())) for t in ("tie2", "in2", "out2", "tie1", "in1", "out1")}
    print(f"dubins_ties (piecewise={piecewise}): hits / edges {n}")
    assert n["tie2"] == (0, 24) and n["in2"] == (24, 24) and n["out2"] == (0, 24)
    assert n["tie1"][0] == n["in1"][0] == n["out1"][0] == 0
    # stage 1 alone: the chord against radius + robot_radius + 2 r_min is an exact tie / a hit / a miss as built
    chord = oracle.edges_check_batch(ps, S[:, :3], G[:, :3], s.robot_radius + 2 * M.R_MIN)[0]
    assert not chord[tags == "tie1"].any() and chord[tags == "in1"].all() and not chord[tags == "out1"].any()


def test_dubins_screen_cases_hit_below_the_radius(oracle):
    s, S, G, which, delta = M.dubins_screen_cases()
    ps = oracle.PolygonSet(s.polys, kinds=s.kinds, paths=s.paths)
    r = oracle.dubins_edges_batch(S, G, M.R_MIN, ps, s.robot_radius, has_time=True, piecewise=True)
    for w in ("R2", "R1"):
        print("screens", w, {d: int(r["hit"][(which == w) & (delta == d)].sum()) for d in M.DELTAS}, "of", int(((which == w) & (delta == 0)).sum()))
    assert r["hit"][(which == "R2") & (delta < 0)].all() and (delta < 0).sum() >= 60
    assert not r["hit"][delta > 0].any() and not r["hit"][which == "R1"].any()
    chord = oracle.edges_check_batch(ps, S[:, :3], G[:, :3], s.robot_radius + 2 * M.R_MIN)[0]
    assert chord[(which == "R1") & (delta < 0)].all() and not chord[(which == "R1") & (delta > 0)].any()


@pytest.mark.parametrize("piecewise", [True, False])
def test_dubins_curved_cases_hit_beyond_stage_2s_radius(oracle, piecewise):
    """the loop reaches obstacles whose path box lies farther than R2 from the chord's box: only the 2 r_min in stage
    1a's radius keeps them"""
    s, S, G, side, gap = M.dubins_curved_cases()
    ps = s.polygon_set(oracle)
    r = oracle.dubins_edges_batch(S, G, M.R_MIN, ps, s.robot_radius, has_time=True, piecewise=piecewise)
    print("curved:", {(sd, g): int(r["hit"][(side == sd) & (gap == g)].sum()) for sd in (-1.0, 1.0) for g in M.CURVED_GAPS}, "of 4 each")
    assert (r["word"] == b"rsr").all() and (r["traj_len"] > 60).all()
    assert r["hit"][(side < 0) & (gap <= 3.5)].all() and not r["hit"][(side > 0) | (gap > 4.0)].any()
    assert gap.min() > 1.4 * (1.5 + s.robot_radius)             # every gap is well beyond R2 (1 + 1e-9)


@pytest.mark.parametrize("dubins", [False, True])
def test_sweep_scene_plants_nodes_on_the_ranges(oracle, dubins):
    """around every query of every obstacle, the one-row path's included: nodes exactly at the range are not listed
    (unless the next segment's ball holds them), a quarter inside they are, and each owns a mirrored edge"""
    sc = M.sweep_scene(dubins)
    s, pts, es = sc["scene"], sc["pts"], sc["es"]
    assert len(pts) <= 1500 and len(es) > 2000
    tree = oracle.KDTree(4, wraps=[3], wrap_points=[2 * np.pi]) if dubins else oracle.KDTree(3)
    tree.insert_many(pts)
    ps = oracle.PolygonSet(s.polys, kinds=s.kinds, paths=s.paths)
    for j in s.moving:
        inside = set(oracle.points_in_conflict_polygon(tree, ps, j, M.SWEEP_RR, M.SWEEP_DELTA, True, dubins).tolist())
        listed = M.sweep_listed(sc, j, dubins)
        assert all((node in inside) == want for node, want in listed.items())
        n = {k: [node for node, name in sc["planted"][j] if name == k] for k in ("at", "in", "out")}
        out = {k: sum(node not in inside for node in v) for k, v in n.items()}
        print(f"sweep ({'dubins' if dubins else 'plane'}): obstacle {j}, {len(sc['queries'][j])} queries: {len(inside)} nodes in "
              f"conflict; planted at / in / out {[len(n[k]) for k in ('at', 'in', 'out')]}, not listed {[out[k] for k in ('at', 'in', 'out')]}")
        assert len(n["at"]) >= 6 * len(sc["queries"][j]) and out["in"] == 0
        assert out["at"] >= 6 and out["out"] >= 6                # (the others lie inside a neighbouring segment's ball)
        if len(sc["queries"][j]) == 1:
            assert out["at"] == len(n["at"]) and out["out"] == len(n["out"])
        assert all((es == node).sum() >= 1 for k in n for node in n[k])
    in0 = oracle.points_in_conflict_polygon(tree, ps, 0, M.SWEEP_RR, M.SWEEP_DELTA, True, dubins)
    assert 0 in in0 and 1 not in in0                             # the root by `<=`, its twin not
    with pytest.raises(RuntimeError):                            # a static obstacle in a space with time
        oracle.points_in_conflict_polygon(tree, ps, 4, M.SWEEP_RR, M.SWEEP_DELTA, True, dubins)
