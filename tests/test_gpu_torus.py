"""The wrapped searches on the lattice tori of tests/torus_model.py, up to three wrapped dimensions and eight copies per
query, against the oracle with == (tests/test_torus_scenes.py holds the oracle to the plain restatement of the ghost
rule and the scenes to the cases they are there for).  The rule is written out five times in the library -- nn_pack
with seen_by_earlier_slot, the two nearest kernels, the self joins, the host's ghost queries of the polygon sweeps --
and this file runs the four that search the tree: rrtx_nn_radius under its switches and batch sizes, the same context
across set_wrap and nodes_append, rrtx_nn_nearest three ways, the fused Dubins preamble and findNewTarget in
[x y t theta] with theta and t wrapped, and the polygon sweeps on a planar torus.

Beside the spaces the scenes T3 / T3r / T2 / T4 / D4 there are T3s / T3sr (two periods of 4: only there does the order
of the wraps change which copy finds a node first) and the side scenes (nodes just below 0 in a wrapped dimension:
only there do the strict side test of a query at period / 2 and a ghost exactly on the skip threshold decide a result)."""
import importlib.util
import os

import numpy as np
import pytest

import torus_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "soak_torus", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "soak_torus.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

SEARCH = ["T3", "T3r", "T2", "T4", "T3s", "T3sr"]
_REF = {}


def _scene(name):
    if name.startswith("side"):
        return M.side_scene(int(name[4:]))
    return M.scene(name)


def _ref(name):
    if name not in _REF:
        _REF[name] = S.Ref(_scene(name))
    return _REF[name]


def _options(cull, filt, tune):
    return ((_capi.RRTX_OPT_NN_CULL, cull), (_capi.RRTX_OPT_NN_FILTER, filt), (_capi.RRTX_OPT_TUNE, tune))


@pytest.mark.parametrize("cull,filt,tune", S.SWITCHES)
@pytest.mark.parametrize("name", SEARCH + ["side0", "side1"])
def test_nn_radius(oracle, name, cull, filt, tune):
    sc, ref = _scene(name), _ref(name)
    with S.make_ctx(sc, _options(cull, filt, tune)) as ctx:
        assert ctx.stats().n_wraps == len(sc["wraps"])
        total = S.check_radius(ctx, sc, ref, f"{name} cull={cull} filter={filt} tune={tune}",
                               batches=S.BATCHES if (filt, tune) == (1, 0) else ())
    assert total > 0


@pytest.mark.parametrize("name", ["T3", "T4"])
def test_nn_radius_lists_outgrow_their_buckets(oracle, name):
    """RRTX_OPT_BUCKET_MULT at its default and no more room than the lists need: the buckets are twice the mean list, and
    one query in eight at r = 3.75 among seven at r = 1.25 has a list of many times the mean"""
    sc, ref = _scene(name), _ref(name)
    nq = len(sc["Q"])
    r = np.where(np.arange(nq) % 8 == 0, 3.75, 1.25)
    want = oracle.range_batch(ref.trees, sc["Q"], r, nearest=False)
    n = np.diff(want["offsets"])
    assert n.max() > 4 * (n.sum() / nq)
    with S.make_ctx(sc) as ctx:
        assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == 2
        S.assert_lists(ctx.nn_radius(sc["Q"], r, cap=len(want["idx"])), want, f"{name} one in eight at 3.75")
        full = ref.lists(3.75)
        S.assert_lists(ctx.nn_radius(sc["Q"], 3.75, cap=len(full["idx"])), full, f"{name} r=3.75, exact capacity")


def test_nn_radius_dev(oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    sc, ref = _scene("T3s"), _ref("T3s")
    nq = len(sc["Q"])
    want = ref.lists(3.25)
    cap = len(want["idx"]) + 7
    with S.make_ctx(sc) as ctx:
        d_q = torch.from_numpy(np.array(sc["Q"])).to(dev)
        d_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        d_idx = torch.empty(cap, dtype=torch.int32, device=dev)
        d_dist = torch.empty(cap, dtype=torch.float64, device=dev)
        d_need = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.nn_radius_dev(d_q.data_ptr(), 3.25, nq, d_off.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), cap, d_need.data_ptr())
        ctx.sync()
        k = int(d_need.item())
        assert k == len(want["idx"])
        S.assert_lists((d_off.cpu().numpy(), d_idx.cpu().numpy()[:k], d_dist.cpu().numpy()[:k]), want, "T3s nn_radius_dev")


def _fresh_lists(oracle, dim, wraps, periods, nodes, Q, r):
    t = oracle.TreeSet(dim, nodes, wraps=list(wraps), wrap_points=list(periods))
    return oracle.range_batch(t, Q, r, nearest=False)


def test_one_context_across_set_wrap(oracle):
    """a third wrap added after a two-wrap call, then a period set again on a dimension that is wrapped already; after
    each change the context equals a fresh oracle tree.  The last state is T3 itself."""
    sc = _scene("T3")
    nodes, Q = sc["nodes"], sc["Q"]
    with Context(3) as ctx:
        ctx.set_wrap(0, 8.0)
        ctx.set_wrap(1, 8.0)
        ctx.nodes_append(nodes)
        for r in (2.5, sc["r_mix"]):
            S.assert_lists(ctx.nn_radius(Q, r), _fresh_lists(oracle, 3, (0, 1), (8.0, 8.0), nodes, Q, r), "two wraps")
        ctx.set_wrap(2, 8.0)
        assert ctx.stats().n_wraps == 3
        for r in (2.5, sc["r_mix"]):
            S.assert_lists(ctx.nn_radius(Q, r), _fresh_lists(oracle, 3, (0, 1, 2), (8.0, 8.0, 8.0), nodes, Q, r), "third wrap")
        ctx.set_wrap(1, 4.0)
        assert ctx.stats().n_wraps == 3
        for name, r in S.radii_of(sc):
            S.assert_lists(ctx.nn_radius(Q, r), _ref("T3").lists(r), f"period set again, r={name}")
        idx, dist = ctx.nn_nearest(Q)
        S.check_nearest_result(sc, _ref("T3"), idx, dist, "period set again")


def test_a_fourth_wrap_is_refused_and_changes_nothing(oracle):
    sc, ref = _scene("T4"), _ref("T4")
    with S.make_ctx(sc) as ctx:
        with pytest.raises(RrtxError) as err:
            ctx.set_wrap(1, 4.0)
        assert err.value.code == _capi.RRTX_E_CAPACITY
        assert ctx.stats().n_wraps == 3
        ctx.set_wrap(3, 8.0)                                   # a dimension that is wrapped already is still accepted
        for name, r in S.radii_of(sc)[1::2]:
            S.assert_lists(ctx.nn_radius(sc["Q"], r), ref.lists(r), f"T4 after the refused wrap, r={name}")


@pytest.mark.parametrize("name", ["T3", "T4"])
def test_nodes_appended_between_calls(oracle, name):
    """the culled search keeps the nodes appended since its last rebuild in a tail; pieces of 1, 5, 600 and the rest cross
    both"""
    sc = _scene(name)
    nodes, Q = sc["nodes"], sc["Q"][:64]
    with Context(sc["dim"], node_capacity=64) as ctx:
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
        for d, per in zip(sc["wraps"], sc["periods"]):
            ctx.set_wrap(d, per)
        done = 0
        for upto in (1, 6, 606, 1900, 1901, len(nodes)):
            ctx.nodes_append(nodes[done:upto])
            done = upto
            for r in (3.25, sc["r_mix"][:64]):
                want = _fresh_lists(oracle, sc["dim"], sc["wraps"], sc["periods"], nodes[:upto], Q, r)
                S.assert_lists(ctx.nn_radius(Q, r), want, f"{name}, {upto} nodes")


@pytest.mark.parametrize("name", SEARCH + ["D4", "side0", "side1"])
def test_nn_nearest(oracle, name):
    S.check_nearest(_scene(name), _ref(name), name)


@pytest.mark.parametrize("has_time", [False, True])
def test_dubins_extend_and_find_target(oracle, has_time):
    total = S.check_dubins(_scene("D4"), _ref("D4"), "D4", has_time=has_time)
    assert total > 10_000


# Found by scene 15 of tools/soak_torus.py (a lattice Dubins space with time): the edge ends on a left turn whose circle
# (centre (0.25, 3.75), radius 0.5) holds the triangle's vertex (0.25, 3.5) at exactly r_min - robot radius from its
# centre, so the arc itself keeps exactly the robot radius from the vertex and only the chords of the stored polyline
# come nearer: the last piece, (0.22624185697781227, 3.2502263441762493) -> the end node, has segmentDistSqrd =
# 0.062494327764345055 < 0.0625 to two sides of the triangle.  Polyline, cost (4.20962102797377), word (lrl) and row
# count (81) equal the oracle's, and the oracle's check on the device's own polyline says hit; the device said no.
LAST_PIECE_S = [1.5, 2.0, 0.25, np.pi / 4]
LAST_PIECE_G = [0.25, 3.25, 1.75, 2.0 * np.pi]
LAST_PIECE_POLYS = [[[0.5, 3.75], [1.0, 3.75], [1.0, 4.5], [0.5, 4.5]], [[0.25, 1.25], [1.25, 1.25], [0.25, 1.5]],
                    [[0.25, 0.5], [1.25, 0.5], [1.25, 0.75], [0.25, 0.75]], [[0.25, 3.5], [1.0, 3.5], [0.25, 4.0]],
                    [[3.0, 3.5], [3.25, 3.5], [3.25, 4.25], [3.0, 4.25]], [[2.75, 3.0], [3.25, 3.0], [2.75, 3.5]]]


@pytest.mark.parametrize("polys", ["all six", "the triangle alone"])
@pytest.mark.parametrize("mode", ["flat", "time, start before end", "time, valid move"])
def test_dubins_last_piece_cuts_inside_the_turning_circle(oracle, mode, polys):
    """In the space with time rrtx_dubins_edges_check returned hit 0 where the oracle returns 1 -- with the soak's six
    polygons and with the triangle alone, for the soak's own edge (start time before end time, an invalid move: flag
    byte 2 from rrtx_extend_candidates_dubins where the oracle has 3) and with the two times exchanged (a valid move).
    The cause was the arc screen of wave_dubins_collides: the last arc of this lrl edge has ONE row, so the polyline's
    last piece is the join that belongs to the middle arc, and with time its far end is the end node instead of the
    tangent point -- outside the middle arc's disk, whose centre is 0.750076 > r_min + robot radius from the triangle.
    The piece that owns such a last piece now keeps every marked obstacle.  Without time the stored polyline keeps
    its own last row, no piece comes within the robot radius, and both sides say 0."""
    has_time = mode != "flat"
    s, g = np.array([LAST_PIECE_S]), np.array([LAST_PIECE_G])
    if mode == "time, valid move":
        s[0, 2], g[0, 2] = g[0, 2], s[0, 2]
    pl = [np.array(p) for p in (LAST_PIECE_POLYS if polys == "all six" else LAST_PIECE_POLYS[3:4])]
    ps = oracle.PolygonSet(pl)
    want = oracle.dubins_edges_batch(s, g, S.RMIN, ps, S.RR, has_time=has_time, piecewise=has_time,
                                     v_min=S.VMIN if has_time else 0.0, v_max=S.VMAX if has_time else 0.0)
    assert want["hit"][0] == (1 if has_time else 0) and want["word"][0] == b"lrl" and want["traj_len"][0] == 81
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * np.pi)
        ctx.nodes_append(s)
        ctx.polygons_set(pl)
        if has_time:
            ctx.set_space_has_time(True)
            ctx.set_dubins_velocity(S.VMIN, S.VMAX)
        cost, word, hit, rows = ctx.dubins_edges_check(s, g, S.RMIN, S.RR)
    print(f"{mode}, {polys}: device cost {cost[0]!r} word {word[0]} hit {hit[0]} rows {rows[0]}; oracle hit {want['hit'][0]}")
    assert cost[0] == want["cost"][0] and word[0] == want["word"][0] and rows[0] == want["traj_len"][0]
    assert (hit[0] & 1) == want["hit"][0]


def test_polygon_sweeps_on_a_planar_torus(oracle):
    sc = M.planar_scene()
    want = S.check_sweeps(sc, "planar torus")
    # the scene, on the reference alone: nodes exactly on a ghost query's range, and edges that are returned only because
    # the copy that shifts both dimensions finds their start node
    on_range = last_copy = 0
    for j, (c, r) in enumerate(zip(sc["centres"], sc["ranges"])):
        q = np.array([[c[0], c[1], 0.0]])
        lists = M.range_lists(sc["nodes"], q, float(r), sc["wraps"], sc["periods"])
        slot = np.full(len(sc["nodes"]), -1)
        slot[lists["idx"]] = lists["slot"]
        assert set(sc["es"][want[j]].tolist()) <= set(lists["idx"].tolist())
        last_copy += int((slot[sc["es"][want[j]]] == 3).sum())
        dist, _ = M.reach(sc["nodes"], q, float(r), sc["wraps"], sc["periods"])
        on_range += int(((dist[1:, 0] == r) & M.searched(q, float(r), sc["wraps"], sc["periods"])[1:]).sum())
    print(f"planar torus: {sum(len(w) for w in want)} edges, {last_copy} through the last copy, {on_range} nodes on a ghost's range")
    assert last_copy >= 16 and on_range >= 16


def test_what_stays_refused_in_a_wrapped_space(oracle):
    sc = _scene("T3")
    with S.make_ctx(sc) as ctx:
        for call in (lambda: ctx.nn_knearest(sc["Q"][:4], 3), lambda: ctx.find_new_target(sc["Q"][:4], 1.25, 4.0, 0.25, lmc=np.zeros(len(sc["nodes"]))),
                     lambda: ctx.extend_candidates(sc["Q"][:4], 1.25, 0.25), lambda: ctx.extend_candidates_self(sc["Q"][:4], 1.25, 0.25)):
            with pytest.raises(RrtxError) as err:
                call()
            assert err.value.code == _capi.RRTX_E_STATE
