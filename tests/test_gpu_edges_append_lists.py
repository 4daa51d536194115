"""The extend lists become mirror edges on the device (rrtx_graph_edges_append_lists_dev, rrtx_graph_edges_append_lists,
rrtx_graph_edges_append_selected, rrtx_graph_edges_get) against the existing sequence rrtx_graph_edges_append +
rrtx_graph_edges_set_dist + rrtx_graph_edges_block on a second context, fed with the arrays of
tests/edges_from_lists_model.py.  Every comparison is exact: np.array_equal, costs as bit patterns.  The conditions on
the inputs (blocked shares, empty and long rows, dropped entries) are asserted on the reference lists alone, before any
device comparison, so no test passes by being empty.

Scene: 2 000 nodes in [-20, 20]^3 (among them a cluster of 70 around the origin and one lone node far outside), 24
spheres, 301 samples: sample 0 at the cluster (a row longer than 64 entries at every radius), sample 1 next to the lone
node with a small sphere beside the middle of the edge between the two (a row whose only edge is blocked both ways), samples 2 .. 6 far from
everything (empty rows).  The radii put the mean row length into each of the four group widths of the list walk
(means of about 4, 12, 24 and 100 entries: groups of 8, 16, 32 and 64 lanes)."""
import json
import math
import os

import numpy as np
import pytest

from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from edges_from_lists_model import edges_from_lists, feed_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
RR = 0.5
W = 20.0
N_TREE, NQ = 2000, 301
LONE = np.array([W + 30.0, 0.0, 0.0])
RADII = {8: 3.4, 16: 4.8, 32: 6.2, 64: 10.2}      # group width of the walk -> ball radius
FORMS = ("dev", "host", "selected")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _scene():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-W, W, (N_TREE, 3))
    pts[-70:] = rng.uniform(-0.4, 0.4, (70, 3))
    pts[-71] = LONE
    sph = np.empty((24, 4))
    k = 0
    while k < 23:                                   # away from the cluster, so that sample 0 is safe
        c = rng.uniform(-W, W, 3)
        if np.linalg.norm(c) > 7.0:
            sph[k] = [*c, rng.uniform(2.0, 3.5)]
            k += 1
    # beside the middle of the unit edge lone node -- sample 1: the reference's distancePointToSegment divides the dot
    # product by the edge's length, not its square, so only an edge this short is tested at its own middle; both ends
    # are clear of the sphere (0.781 against 0.7), the middle is not (0.6)
    sph[23] = [*(LONE + [0.5, 0.6, 0.0]), 0.2]
    Q = rng.uniform(-W, W, (NQ, 3))
    Q[0] = [0.05, -0.03, 0.02]
    Q[1] = LONE + [1.0, 0.0, 0.0]
    Q[2:7] = np.array([-W - 40.0, 0.0, 0.0]) - 5.0 * np.arange(5)[:, None] * np.array([1.0, 0.0, 0.0])
    child = np.arange(1, N_TREE)
    par = (rng.random(N_TREE - 1) * child).astype(np.int32)
    return pts, sph, Q, child.astype(np.int32), par


SCENE = _scene()


def _context(with_tree_edges=True):
    pts, sph, _, child, par = SCENE
    ctx = Context(3)
    ctx.nodes_append(pts)
    ctx.spheres_set(sph)
    if with_tree_edges:
        ctx.graph_edges_append(child, par)
    return ctx


def _node_of(unsafe, n_nodes):
    ins = (unsafe == 0) & (np.arange(len(unsafe)) % 7 != 6)
    node_of = np.full(len(unsafe), -1, dtype=np.int32)
    node_of[ins] = n_nodes + np.arange(int(ins.sum()), dtype=np.int32)
    return node_of, ins


def _cost_in(lists):
    return lists["cost_in"] if "cost_in" in lists else lists["cost"]


def _cost_out(lists):
    return lists["cost_out"] if "cost_out" in lists else lists["cost"]


def _model(lists, node_of, batch=False):
    return edges_from_lists(lists["offsets"], lists["idx"], _cost_out(lists), _cost_in(lists), lists["hit_out"],
                            lists["hit_in"], node_of, batch)


def _assert_same_mirror(a, b, what=""):
    assert a.n_graph_edges == b.n_graph_edges, what
    ga, gb = a.graph_edges_get(), b.graph_edges_get()
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]), (what, "start / end")
    assert np.array_equal(_bits(ga[2]), _bits(gb[2])), (what, "dist")
    assert np.array_equal(_bits(ga[3]), _bits(gb[3])), (what, "dist_original")
    return ga


def _assert_same_costs(a, b, update, what=""):
    la, pa, _ = a.graph_cost_to_root(0, update=update)
    lb, pb, _ = b.graph_cost_to_root(0, update=update)
    assert np.array_equal(_bits(la), _bits(lb)) and np.array_equal(pa, pb), (what, "lmc / parent_edge")
    return lb, pb


def _dev_lists(torch, lists, node_of, cap_extra=3):
    """The host lists uploaded as the *_dev extend calls leave them: arrays of cap entries, the count in a device word."""
    n = len(lists["idx"])
    cap = n + cap_extra
    dev = torch.device("cuda", 0)

    def up(a, dtype, fill):
        t = torch.full((max(cap, 1),), fill, dtype=dtype, device=dev)
        if n:
            t[:n] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t
    d = dict(off=torch.from_numpy(np.ascontiguousarray(lists["offsets"])).to(dev), idx=up(lists["idx"], torch.int32, -7),
             co=up(_cost_out(lists), torch.float64, -7.0), ho=up(lists["hit_out"], torch.uint8, 7),
             hi=up(lists["hit_in"], torch.uint8, 7), need=torch.tensor([n], dtype=torch.int64, device=dev),
             node_of=torch.from_numpy(node_of).to(dev), rows=torch.full((len(node_of) + 1,), -7, dtype=torch.int64, device=dev),
             cap=cap)
    d["ci"] = d["co"] if "cost_in" not in lists else up(lists["cost_in"], torch.float64, -7.0)
    torch.cuda.synchronize()
    return d


def _append_dev(ctx, d, nq, batch=False, cap=None, need=True):
    first, added = ctx.graph_edges_append_lists_dev(nq, d["off"].data_ptr(), d["idx"].data_ptr(), d["co"].data_ptr(),
                                                    d["ci"].data_ptr(), d["ho"].data_ptr(), d["hi"].data_ptr(),
                                                    d["need"].data_ptr() if need else None, d["cap"] if cap is None else cap,
                                                    d["node_of"].data_ptr(), batch, d["rows"].data_ptr())
    ctx.sync()
    return first, added, d["rows"].cpu().numpy()


# ---- the three forms against the existing sequence, at the four group widths ------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("group", sorted(RADII))
def test_forms_match_the_existing_sequence(group, form):
    torch = pytest.importorskip("torch")
    pts, sph, Q, _, _ = SCENE
    r = RADII[group]
    rng = np.random.default_rng(11)
    lmc_in = rng.uniform(0.0, 60.0, N_TREE)
    lmc_in[0] = 0.0
    with _context() as ref, _context() as ctx:
        lists = ref.extend_candidates(Q, r, RR)
        node_of, ins = _node_of(lists["sample_unsafe"], N_TREE)
        # ---- the reference lists alone
        rows = np.diff(lists["offsets"])
        mean = int(lists["offsets"][NQ]) // NQ
        print(f"group {group}: {len(lists['idx'])} entries, mean {mean}, longest row {rows.max()}, {int(ins.sum())} inserted, "
              f"out blocked {np.mean(lists['hit_out'] != 0):.3f}, in blocked {np.mean(lists['hit_in'] != 0):.3f}")
        assert (group == 8 and mean <= 8) or (group > 8 and group // 2 < mean <= group) or (group == 64 and mean > 32)
        assert rows[0] > 64 and ins[0] and (rows == 0).sum() >= 5
        assert NQ % 2 == 1 and (lists["sample_unsafe"] != 0).sum() >= 3 and (node_of < 0).sum() > NQ // 7
        assert np.mean(lists["hit_out"] != 0) >= 0.05 and np.mean(lists["hit_in"] != 0) >= 0.05
        all_in_blocked = [j for j in range(NQ) if ins[j] and rows[j] > 0 and
                          (lists["hit_in"][lists["offsets"][j]:lists["offsets"][j + 1]] != 0).all()]
        assert 1 in all_in_blocked
        model = _model(lists, node_of)
        assert model["blocked"].sum() > 0 and len(model["start"]) > len(lists["idx"]) // 2
        # ---- both contexts get the inserted samples, the reference the model's arrays through the existing calls
        ref.nodes_append(Q[ins])
        first_ref = feed_reference(ref, model)
        assert first_ref == N_TREE - 1
        if form == "selected":
            sel = ctx.extend_select(Q, r, RR, lmc=lmc_in)
            assert np.array_equal(sel["sample_unsafe"], lists["sample_unsafe"]) and sel["n_neighbors"] == len(lists["idx"])
            ctx.nodes_append(Q[ins])
            ctx.node_cost_set(0, [0.0])                               # the calls that keep the lists
            assert ctx.n_graph_edges == N_TREE - 1 and ctx.get_option(_capi.RRTX_OPT_NN_CULL) >= 0
            first, added, row_first = ctx.graph_edges_append_selected(node_of)
        elif form == "host":
            ctx.nodes_append(Q[ins])
            first, added, row_first = ctx.graph_edges_append_lists(lists["offsets"], lists["idx"], lists["cost"], lists["cost"],
                                                                   lists["hit_out"], lists["hit_in"], node_of)
        else:
            ctx.nodes_append(Q[ins])
            first, added, row_first = _append_dev(ctx, _dev_lists(torch, lists, node_of), NQ)
        assert first == first_ref and added == len(model["start"])
        assert row_first.dtype == np.int64 and np.array_equal(row_first, model["row_first"])
        _assert_same_mirror(ctx, ref, (group, form))
        lmc, par = _assert_same_costs(ctx, ref, False, (group, form))
        assert np.isfinite(lmc[N_TREE:]).sum() > ins.sum() // 2 and (par >= first).sum() > 10
        # ---- a burst of new spheres swept over both mirrors, then a burst of the old ones released
        new = np.array([[*Q[8], 2.5], [*Q[9], 3.0], [*Q[10], 2.0]])
        both = np.concatenate([sph, new])
        search = both[:, 3] + RR + max(r, 1.0) + 1.0
        got = []
        for c in (ctx, ref):
            c.spheres_set(both)
            got.append(c.obstacle_sweep_batch([24, 25, 26], search[24:], RR, block=True))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (group, form, "sweep")
        assert (got[1][1] >= first).sum() > 0
        _assert_same_costs(ctx, ref, True, (group, form, "after the sweep"))
        leaving = np.array([0, 1, 2, 3, 4, 5, 23, 24], dtype=np.int32)
        got = [c.obstacle_release_batch(leaving, search[leaving], RR, unblock=True) for c in (ctx, ref)]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (group, form, "release")
        freed = got[1][1]
        assert (freed >= first).sum() > 0 and model["blocked"][freed[freed >= first] - first].any()   # edges blocked at the append
        _assert_same_costs(ctx, ref, True, (group, form, "after the release"))
        _assert_same_mirror(ctx, ref, (group, form, "at the end"))


# ---- the lists of the batch among itself: idx holds batch positions ------------------------------------------------
@pytest.mark.parametrize("form", ("dev", "host"))
def test_self_lists(form):
    torch = pytest.importorskip("torch")
    _, _, Q, _, _ = SCENE
    r = RADII[32]
    with _context() as ref, _context() as ctx:
        unsafe = ref.extend_candidates(Q, r, RR)["sample_unsafe"]
        lists = ref.extend_candidates_self(Q, r, RR, skip=unsafe)
        node_of, ins = _node_of(unsafe, N_TREE)
        model = _model(lists, node_of, batch=True)
        print(f"self lists: {len(lists['idx'])} entries, {model['dropped']} dropped, {len(model['start'])} edges")
        # (no blocked edge is asked for here: both ends of a same-batch edge are safe samples, and the reference's
        # distancePointToSegment tests an edge longer than a unit next to an end only)
        assert len(lists["idx"]) > 200 and model["dropped"] >= 1 and 0 < len(model["start"]) < 2 * len(lists["idx"])
        for c in (ref, ctx):
            c.nodes_append(Q[ins])
        first_ref = feed_reference(ref, model)
        if form == "host":
            first, added, row_first = ctx.graph_edges_append_lists(lists["offsets"], lists["idx"], lists["cost"], lists["cost"],
                                                                   lists["hit_out"], lists["hit_in"], node_of, idx_is_batch=True)
        else:
            first, added, row_first = _append_dev(ctx, _dev_lists(torch, lists, node_of), NQ, batch=True)
        assert first == first_ref and added == len(model["start"]) and np.array_equal(row_first, model["row_first"])
        s, e, _, _ = _assert_same_mirror(ctx, ref, ("self", form))
        assert s[first:].min() >= N_TREE and e[first:].min() >= N_TREE        # every edge joins two samples of the batch
        _assert_same_costs(ctx, ref, False, ("self", form))


# ---- Dubins lists: cost_out != cost_in, flag bytes of value 2, straight from the device call ------------------------
def test_dubins_lists_from_the_device():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(23)
    env = json.load(open(os.path.join(ROOT, "golden", "env_inputs.json")))
    polys = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_polygons"]][::-1][:12]
    paths = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_paths"]][::-1][:12]
    n, nq, r, r_min = 1000, 128, 16.0, 2.0
    pts = np.concatenate([rng.uniform(-50.0, 50.0, (n, 2)), rng.uniform(10.0, 35.0, (n, 1)), rng.uniform(0.0, 2.0 * math.pi, (n, 1))], axis=1)
    Q = np.concatenate([rng.uniform(-50.0, 50.0, (nq, 2)), rng.uniform(10.0, 35.0, (nq, 1)), rng.uniform(0.0, 2.0 * math.pi, (nq, 1))], axis=1)

    def context():
        c = Context(4)
        c.set_wrap(3, 2.0 * math.pi)
        c.nodes_append(pts)
        c.polygons_set(polys, kinds=[6] * len(polys), paths=paths)
        c.set_space_has_time(True)
        c.set_dubins_velocity(5.0, 30.0)
        return c
    with context() as ref, context() as ctx:
        lists = ref.extend_candidates_dubins(Q, r, RR, r_min)
        k = len(lists["idx"])
        node_of, ins = _node_of(lists["sample_unsafe"], n)
        model = _model(lists, node_of)
        print(f"dubins: {k} entries, {len(model['start'])} edges, {int(model['blocked'].sum())} blocked out-edges")
        assert k > 300 and not np.array_equal(lists["cost_out"], lists["cost_in"])
        assert (lists["hit_out"] == 2).any() and (lists["hit_in"] == 2).any()
        ref.nodes_append(Q[ins])
        first_ref = feed_reference(ref, model)
        dev = torch.device("cuda", 0)
        t = lambda m, dt: torch.zeros((max(m, 1),), dtype=dt, device=dev)
        cap = k + 5
        off, idx, key, co, ci = t(nq + 1, torch.int64), t(cap, torch.int32), t(cap, torch.float64), t(cap, torch.float64), t(cap, torch.float64)
        ho, hi, need = t(cap, torch.uint8), t(cap, torch.uint8), t(1, torch.int64)
        ni, nd, un = t(nq, torch.int32), t(nq, torch.float64), t(nq, torch.uint8)
        dq = torch.from_numpy(Q).to(dev)
        torch.cuda.synchronize()
        ctx.extend_candidates_dubins_dev(dq.data_ptr(), nq, r, RR, r_min, off.data_ptr(), idx.data_ptr(), key.data_ptr(),
                                         co.data_ptr(), ci.data_ptr(), None, None, ho.data_ptr(), hi.data_ptr(), cap,
                                         need.data_ptr(), ni.data_ptr(), nd.data_ptr(), un.data_ptr())
        ctx.sync()
        assert int(need.item()) == k
        ctx.nodes_append(Q[ins])                     # the lists are against the tree as it stood
        d = dict(off=off, idx=idx, co=co, ci=ci, ho=ho, hi=hi, need=need, cap=cap, node_of=torch.from_numpy(node_of).to(dev),
                 rows=t(nq + 1, torch.int64))
        first, added, row_first = _append_dev(ctx, d, nq)
        assert first == first_ref == 0 and added == len(model["start"]) and np.array_equal(row_first, model["row_first"])
        _, _, dist, dist0 = _assert_same_mirror(ctx, ref, "dubins")
        assert np.isinf(dist[model["blocked"]]).all() and np.array_equal(_bits(dist0), _bits(model["cost"]))
        _assert_same_costs(ctx, ref, False, "dubins")


# ---- the append crosses a capacity step of the mirror ----------------------------------------------------------------
def test_growth_keeps_the_earlier_edges():
    _, _, Q, _, _ = SCENE
    rng = np.random.default_rng(3)
    es, ee = rng.integers(0, N_TREE, 4000).astype(np.int32), rng.integers(0, N_TREE, 4000).astype(np.int32)
    with _context(False) as ref, _context(False) as ctx:
        for c in (ref, ctx):
            assert c.graph_edges_append(es, ee) == 0
            c.graph_edges_block(np.arange(0, 4000, 9, dtype=np.int32))
        before = ctx.graph_edges_get()
        lists = ref.extend_candidates(Q, RADII[16], RR)
        node_of, ins = _node_of(lists["sample_unsafe"], N_TREE)
        model = _model(lists, node_of)
        assert 4000 + len(model["start"]) > 4096
        for c in (ref, ctx):
            c.nodes_append(Q[ins])
        feed_reference(ref, model)
        first, added, _ = ctx.graph_edges_append_lists(lists["offsets"], lists["idx"], lists["cost"], lists["cost"],
                                                       lists["hit_out"], lists["hit_in"], node_of)
        assert first == 4000 and added == len(model["start"])
        after = _assert_same_mirror(ctx, ref, "growth")
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b[:4000]) if b.dtype == np.float64 else b[:4000])
        # a gather of ids, and a range in the middle
        ids = np.array([4000 + added - 1, 0, 4095, 4096, 17, 17], dtype=np.int32)
        got = ctx.graph_edges_get(ids)
        for g, a in zip(got, after):
            assert np.array_equal(_bits(g) if g.dtype == np.float64 else g, _bits(a[ids]) if a.dtype == np.float64 else a[ids])
        got = ctx.graph_edges_get(first_id=4090, n=20)
        assert np.array_equal(got[0], after[0][4090:4110]) and np.array_equal(_bits(got[2]), _bits(after[2][4090:4110]))
        _assert_same_costs(ctx, ref, False, "growth")


# ---- refusals: the code, and a mirror that is left as it was --------------------------------------------------------
def test_refusals_leave_the_mirror_alone():
    torch = pytest.importorskip("torch")
    _, _, Q, _, _ = SCENE
    r = RADII[16]
    with _context() as ctx:
        lists = ctx.extend_candidates(Q, r, RR)
        node_of, ins = _node_of(lists["sample_unsafe"], N_TREE)
        ctx.nodes_append(Q[ins])
        n_nodes = ctx.n_nodes
        before = ctx.graph_edges_get()

        def refused(code, call):
            with pytest.raises(RrtxError) as ei:
                call()
            assert ei.value.code == code, (ei.value.code, code)
            assert ctx.n_graph_edges == len(before[0])
            for a, b in zip(before, ctx.graph_edges_get()):
                assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)

        args = (lists["offsets"], lists["idx"], lists["cost"], lists["cost"], lists["hit_out"], lists["hit_in"])
        k = len(lists["idx"])
        # the extend call produced more than the lists hold
        refused(_capi.RRTX_E_CAPACITY, lambda: ctx.graph_edges_append_lists(*args, node_of, n_valid=k, cap=k - 1))
        d = _dev_lists(torch, lists, node_of)
        refused(_capi.RRTX_E_CAPACITY, lambda: _append_dev(ctx, d, NQ, cap=k - 1))
        # a near node outside the tree (in a row that is inserted)
        j = int(np.nonzero(ins & (np.diff(lists["offsets"]) > 0))[0][3])
        bad = lists["idx"].copy()
        bad[lists["offsets"][j]] = n_nodes
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_append_lists(args[0], bad, *args[2:], node_of))
        bad[lists["offsets"][j]] = -1
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_append_lists(args[0], bad, *args[2:], node_of))
        d["idx"][int(lists["offsets"][j])] = n_nodes
        refused(_capi.RRTX_E_INVALID, lambda: _append_dev(ctx, d, NQ))
        # ... the same entry in a row that is not inserted is not looked at
        j7 = int(np.nonzero((node_of < 0) & (np.diff(lists["offsets"]) > 0))[0][0])
        ok = lists["idx"].copy()
        ok[lists["offsets"][j7]] = n_nodes
        model = _model(lists, node_of)
        first, added, _ = ctx.graph_edges_append_lists(args[0], ok, *args[2:], node_of)
        assert added == len(model["start"]) and first == len(before[0])
        before = ctx.graph_edges_get()
        # a batch position outside the batch
        bad = lists["idx"].copy()
        bad[lists["offsets"][j]] = NQ
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_append_lists(args[0], bad, *args[2:], node_of, idx_is_batch=True))
        # node_of beyond the node count
        nb = node_of.copy()
        nb[j] = n_nodes
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_append_lists(*args, nb))
        # offsets out of order
        ob = lists["offsets"].copy()
        ob[j] = ob[j + 1] + 1
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_append_lists(ob, *args[1:], node_of))
        # nothing to do
        first, added, rows = ctx.graph_edges_append_lists(*args, np.full(NQ, -1, dtype=np.int32))
        assert added == 0 and first == len(before[0]) and not rows.any()
        first, added, rows = ctx.graph_edges_append_lists([0], [], [], [], [], [], [])
        assert added == 0 and rows.tolist() == [0]
        # a range or an id outside the mirror
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_get(first_id=len(before[0]) - 1, n=2))
        refused(_capi.RRTX_E_INVALID, lambda: ctx.graph_edges_get(np.array([0, len(before[0])], dtype=np.int32)))


def test_selected_needs_the_lists_of_the_last_select():
    _, _, Q, _, _ = SCENE
    r = RADII[16]
    lmc = np.zeros(N_TREE)
    with _context() as ctx:
        before = ctx.n_graph_edges

        def refused(call):
            with pytest.raises(RrtxError) as ei:
                call()
            assert ei.value.code == _capi.RRTX_E_STATE and ctx.n_graph_edges == before

        node_of = np.full(NQ, -1, dtype=np.int32)
        node_of[0] = 5
        refused(lambda: ctx.graph_edges_append_selected(node_of))                    # no select yet
        sel = ctx.extend_select(Q, r, RR, lmc=lmc)
        refused(lambda: ctx.graph_edges_append_selected(node_of[:-1]))               # another nq
        ctx.nn_radius(Q[:4], r)                                                      # a search uses the lists' workspaces
        refused(lambda: ctx.graph_edges_append_selected(node_of))
        ctx.extend_select(Q, r, RR, lmc=lmc)
        ctx.extend_candidates(Q[:8], r, RR)
        refused(lambda: ctx.graph_edges_append_selected(node_of))
        ctx.extend_select(Q, r, RR, lmc=lmc)
        ctx.graph_cost_update_delta(0)                                               # the graph calls keep them
        first, added, rows = ctx.graph_edges_append_selected(node_of)
        assert first == before and added > 64 and rows[0] == 0 and rows[1] == added and rows[-1] == added
        s, e, _, _ = ctx.graph_edges_get(first_id=first)
        assert s[0] == 5 and ((s == 5) | (e == 5)).all() and sel["n_neighbors"] > added // 2
