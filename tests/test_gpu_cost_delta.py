"""rrtx_graph_cost_update_delta: the cost update reported as the nodes it changed, against references that never come
from the code under test.  rrtLMC is the oracle's (tests/mirror_model.py::MirrorModel.solve -- oracle.Graph,
reduceInconsistency); the parent edge is the lowest edge id that attains the oracle's value, worked out in numpy the
way _check_parents of test_gpu_graph_cost.py does; the expected delta is the numpy diff of two consecutive such states
(costs compared as 64-bit patterns, a node never reported counting as +Inf / -1), ascending.  Every comparison is
np.array_equal: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

from mirror_model import MirrorModel
from test_gpu_graph_cost import _edge_dist, _geometric_graph, _oracle_solve

pytestmark = pytest.mark.gpu
INF = float("inf")
RR = 0.5
W = 256          # nodes per compaction workgroup: kDeltaBlock in rrtqx_3d_amd/csrc/kernels_graph.hip
N, R_EDGE, ROOT = 2000, 4.5, 17
SPHERE_RADIUS = 3.0


def _lowest_parent(lmc, s, e, w, root):
    """per node the lowest id among the edges whose one rounded sum attains the node's value (-1: root, orphan)"""
    n = len(lmc)
    fin = np.isfinite(lmc)
    ok = np.isfinite(w) & (w >= 0) & fin[e] & fin[s] & (s != root)
    att = np.nonzero(ok & (np.where(ok, lmc[e] + np.where(ok, w, 0), INF) == lmc[s]))[0]
    lowest = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(lowest, s[att], att)
    par = np.where(lowest == np.iinfo(np.int64).max, -1, lowest).astype(np.int32)
    assert par[root] == -1 and np.all(par[~fin] == -1) and np.all(par[fin & (np.arange(n) != root)] >= 0)
    return par


def _state(model, root):
    lmc, _ = model.solve(root)
    lmc = np.ascontiguousarray(lmc, dtype=np.float64)
    return lmc, _lowest_parent(lmc, model.start, model.end, model.dist, root)


NOTHING = (np.zeros(0), np.zeros(0, dtype=np.int32))


def _delta(prev, now):
    (l0, p0), (l1, p1) = prev, now
    n = len(l1)
    l0 = np.ascontiguousarray(np.concatenate([l0, np.full(n - len(l0), INF)]))
    p0 = np.concatenate([p0, np.full(n - len(p0), -1, dtype=np.int32)])
    ch = np.flatnonzero((l0.view(np.uint64) != l1.view(np.uint64)) | (p0 != p1)).astype(np.int32)
    return ch, l1[ch], p1[ch]


def _assert_delta(got, want, what):
    node, lmc, par = got[:3]
    assert node.dtype == np.int32 and lmc.dtype == np.float64 and par.dtype == np.int32, what
    assert np.array_equal(node, want[0]), what
    assert np.array_equal(lmc.view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)), what
    assert np.array_equal(par, want[2]), what


def _assert_full(ctx, root, state, what):
    lmc, par, _ = ctx.graph_cost_update(root)
    assert np.array_equal(lmc, state[0]) and np.array_equal(par, state[1]), what


def _raw(ctx, root, store=0, cap=0, arrays=True, parent=True, needed=True):
    """the C call itself: (rc, needed, node, lmc, parent_edge)"""
    node = np.full(max(cap, 1), -7, dtype=np.int32)
    lmc = np.full(max(cap, 1), -7.0)
    par = np.full(max(cap, 1), -7, dtype=np.int32)
    cnt = C.c_int64(-1)
    rc = ctx._lib.rrtx_graph_cost_update_delta(ctx._h, root, store, _capi._ptr(node) if arrays else None,
                                               _capi._ptr(lmc) if arrays else None,
                                               _capi._ptr(par) if arrays and parent else None, cap,
                                               C.byref(cnt) if needed else None, None)
    return rc, cnt.value, node, lmc, par


class Scene:
    """The graph of test_cost_to_root_matches_reduce_inconsistency (2000 uniform nodes, r = 4.5, root 17) and one sphere,
    chosen on the CPU so that blocking what it sweeps changes at least one node and fewer than half of them."""

    def __init__(self, oracle):
        self.oracle = oracle
        rng = np.random.default_rng(N)
        self.pts = rng.uniform(-20, 20, (N, 3))
        self.s, self.e = _geometric_graph(oracle, self.pts, R_EDGE)
        self.range = RR + R_EDGE + SPHERE_RADIUS
        self.sphere = None
        base = self.model()
        self.state0 = _state(base, ROOT)
        for c in (500, 1700, 100, 900, 1300):
            m = self.model(np.array([[*self.pts[c], SPHERE_RADIUS]]))
            ids = m.sweep_row(0, self.range, RR)
            m.block(ids)
            st = _state(m, ROOT)
            if 1 <= len(_delta(self.state0, st)[0]) < N // 2:
                self.sphere, self.blocked, self.state1 = m.cxyzr.copy(), ids, st
                break
        assert self.sphere is not None

    def model(self, sphere=None):
        sphere = self.sphere if sphere is None else sphere
        m = MirrorModel(self.oracle)
        m.nodes_append(self.pts)
        m.append(self.s, self.e)
        m.spheres_set(np.zeros((0, 4)) if sphere is None else sphere)
        return m

    def context(self):
        ctx = Context(3)
        ctx.nodes_append(self.pts)
        ctx.graph_edges_append(self.s, self.e)
        ctx.spheres_set(self.sphere, np.ones(1, dtype=np.uint8))
        return ctx


@pytest.fixture(scope="module")
def scene(oracle):
    return Scene(oracle)


def _replanning_reference(oracle, scene):
    """the steps of test_replanning_sequence on the host model: what is sent to the device, the state after every step
    and the delta every step must report"""
    m = scene.model()
    states, what = [scene.state0], ["first"]
    # the sphere appears; it leaves again
    ids = m.sweep_row(0, scene.range, RR)
    assert np.array_equal(ids, scene.blocked)
    m.block(ids)
    states.append(_state(m, ROOT)); what.append("sweep + block")
    freed = m.release_row(0, scene.range, RR, [0])
    assert np.array_equal(freed, ids)
    m.unblock(freed)
    states.append(_state(m, ROOT)); what.append("release + unblock")
    # the tree grows by 300 nodes and the edges they bring, around the node farthest from the root (nodes spread over
    # the whole world would open shortcuts for most of the tree)
    far = scene.pts[np.argmax(np.where(np.isfinite(scene.state0[0]), scene.state0[0], -1.0))]
    more = np.clip(far + np.random.default_rng(N + 1).uniform(-4, 4, (300, 3)), -20, 20)
    s2, e2 = _geometric_graph(oracle, np.concatenate([scene.pts, more]), R_EDGE)
    new = np.maximum(s2, e2) >= N
    s_new, e_new = s2[new], e2[new]
    m.nodes_append(more)
    m.append(s_new, e_new)
    states.append(_state(m, ROOT)); what.append("append")
    # a run of edges three times as dear
    dear = m.dist[:400] * 3.0
    m.set_dist(0, dear)
    states.append(_state(m, ROOT)); what.append("set_dist")
    # the reference alone: every step changes something, and fewer than half of the nodes
    deltas = [_delta(NOTHING, states[0])] + [_delta(a, b) for a, b in zip(states, states[1:])]
    assert len(deltas[0][0]) == np.isfinite(states[0][0]).sum() > N // 2
    for d, st, name in zip(deltas[1:], states[1:], what[1:]):
        assert 1 <= len(d[0]) < len(st[0]) // 2, (name, len(d[0]))
    assert np.array_equal(states[2][0], states[0][0]) and np.array_equal(states[2][1], states[0][1])
    assert np.array_equal(deltas[2][0], deltas[1][0])                    # the nodes go back to their first values
    assert (deltas[3][0] >= N).any() and (deltas[3][0] < N).any()        # new nodes, and old ones they improve
    return dict(ids=ids, freed=freed, more=more, s_new=s_new, e_new=e_new, dear=dear, states=states, deltas=deltas, what=what)


def test_replanning_sequence(oracle, scene):
    ref = _replanning_reference(oracle, scene)
    ids, freed, more, s_new, e_new, dear = (ref[k] for k in ("ids", "freed", "more", "s_new", "e_new", "dear"))
    states, deltas, what = ref["states"], ref["deltas"], ref["what"]
    with scene.context() as ctx:
        _assert_delta(ctx.graph_cost_update_delta(ROOT), deltas[0], what[0])
        _assert_full(ctx, ROOT, states[0], what[0])
        off, got = ctx.obstacle_sweep_batch([0], scene.range, RR, block=True)
        assert np.array_equal(got, ids)
        _assert_delta(ctx.graph_cost_update_delta(ROOT), deltas[1], what[1])
        _assert_full(ctx, ROOT, states[1], what[1])
        off, got = ctx.obstacle_release_batch([0], scene.range, RR, unblock=True)
        assert np.array_equal(got, freed)
        _assert_delta(ctx.graph_cost_update_delta(ROOT), deltas[2], what[2])
        _assert_full(ctx, ROOT, states[2], what[2])
        ctx.nodes_append(more)
        ctx.graph_edges_append(s_new, e_new)
        _assert_delta(ctx.graph_cost_update_delta(ROOT), deltas[3], what[3])
        _assert_full(ctx, ROOT, states[3], what[3])
        ctx.graph_edges_set_dist(0, dear)
        _assert_full(ctx, ROOT, states[4], what[4])                      # the full-array call first this time
        _assert_delta(ctx.graph_cost_update_delta(ROOT), deltas[4], what[4])
        node, lmc, par, _ = ctx.graph_cost_update_delta(ROOT)            # nothing in between
        assert len(node) == len(lmc) == len(par) == 0
        rc, needed, *_ = _raw(ctx, ROOT, cap=0, arrays=False)
        assert rc == _capi.RRTX_OK and needed == 0
        _assert_full(ctx, ROOT, states[4], "nothing")


def test_capacity_and_argument_errors(scene):
    first = _delta(NOTHING, scene.state0)
    second = _delta(scene.state0, scene.state1)
    k = len(first[0])
    with scene.context() as ctx:
        # one slot short: the count is right, the baseline stays, a call with room returns the whole list
        rc, needed, *_ = _raw(ctx, ROOT, cap=k - 1)
        assert rc == _capi.RRTX_E_CAPACITY and needed == k
        rc, needed, *_ = _raw(ctx, ROOT, cap=0, arrays=False)            # count only: something changed
        assert rc == _capi.RRTX_E_CAPACITY and needed == k
        rc, needed, node, lmc, par = _raw(ctx, ROOT, cap=k)
        assert rc == _capi.RRTX_OK and needed == k
        _assert_delta((node[:k], lmc[:k], par[:k]), first, "exact room")
        rc, needed, *_ = _raw(ctx, ROOT, cap=0, arrays=False)            # count only: nothing changed
        assert rc == _capi.RRTX_OK and needed == 0
        # argument errors: RRTX_E_INVALID, and what was reported still stands
        ctx.graph_edges_block(scene.blocked)
        for kw in (dict(cap=-1), dict(cap=8, arrays=False), dict(cap=0, needed=False)):
            assert _raw(ctx, ROOT, **kw)[0] == _capi.RRTX_E_INVALID, kw
        node = np.zeros(8, dtype=np.int32)
        cnt = C.c_int64()
        assert ctx._lib.rrtx_graph_cost_update_delta(ctx._h, ROOT, 0, _capi._ptr(node), None, None, 8, C.byref(cnt),
                                                     None) == _capi.RRTX_E_INVALID      # lmc NULL alone
        for bad in (-1, N):
            assert _raw(ctx, bad, cap=N)[0] == _capi.RRTX_E_INVALID
        k2 = len(second[0])
        rc, needed, *_ = _raw(ctx, ROOT, cap=k2 - 1)
        assert rc == _capi.RRTX_E_CAPACITY and needed == k2
        # parent_edge may be NULL: the same nodes and costs
        rc, needed, node, lmc, par = _raw(ctx, ROOT, cap=N, parent=False)
        assert rc == _capi.RRTX_OK and needed == k2
        assert np.array_equal(node[:k2], second[0]) and np.array_equal(lmc[:k2], second[1]) and np.all(par == -7)
        assert np.all(node[k2:] == -7)                                   # nothing written beyond the count
        _assert_full(ctx, ROOT, scene.state1, "after the errors")
    with Context(3) as empty:
        assert _raw(empty, 0, cap=4)[0] == _capi.RRTX_E_STATE            # as rrtx_graph_cost_update: an empty tree


def _lattice(n):
    """the lattice of test_lattices_with_a_ragged_last_tile: 64 columns, jittered third coordinate"""
    cols = 64
    rng = np.random.default_rng(n)
    i = np.arange(n)
    pts = np.stack([(i % cols).astype(np.float64), (i // cols).astype(np.float64), rng.uniform(0.0, 0.25, n)], axis=1)
    right = i[(i % cols != cols - 1) & (i + 1 < n)]
    down = i[i + cols < n]
    a = np.concatenate([right, down])
    b = np.concatenate([right + 1, down + cols])
    return pts, np.concatenate([a, b]).astype(np.int32), np.concatenate([b, a]).astype(np.int32)


def _lattice_reference(oracle, n):
    pts, s, e = _lattice(n)
    w = _edge_dist(pts, s, e)
    root = (n // 128) * 64 + 31                              # a node in the middle row
    targets = sorted({0, n - 1} | ({W - 1, W} if n > W else set()))
    assert root not in targets

    def state(w):
        lmc = np.ascontiguousarray(_oracle_solve(oracle, n, s, e, w, root)[0])
        return lmc, _lowest_parent(lmc, s, e, w, root)
    st0 = state(w)
    dear = np.flatnonzero(np.isin(s, targets))
    w1 = w.copy()
    w1[dear] *= 4.0
    st1 = state(w1)
    first, second = _delta(NOTHING, st0), _delta(st0, st1)
    assert np.array_equal(first[0], np.arange(n))
    assert set(targets) <= set(second[0].tolist()) and len(second[0]) < n // 2
    per_group = np.bincount(second[0] // W, minlength=(n + W - 1) // W)
    if n > 2 * W:
        assert (per_group[1:-1] == 0).any() and per_group[0] > 0 and per_group[-1] > 0
    return pts, s, e, root, dear, w1, st1, first, second


@pytest.mark.parametrize("n", [W - 1, W + 1, 5 * W - 1, 5 * W + 1])
def test_workgroup_boundaries(oracle, n):
    """W k +- 1 nodes: 1, 2, 5 and 6 compaction workgroups, the last one ragged (one node in it for W k + 1).  The first
    call reports every node (all workgroups full); then the out-edges of node 0, of node n - 1 and of the two nodes
    either side of the first workgroup boundary (W - 1 | W, where there is one) become four times as dear, which
    changes those nodes and, with 5 W +- 1 nodes, leaves a workgroup in the middle without any changed node.
    (More than 4096 workgroups -- a second round of the scan of the per-workgroup counts -- needs over a million nodes
    and is not built here: it is the 64-bit instantiation of excl_scan_kernel that
    test_gpu_extend_select.py::test_synthetic_lists_across_scan_rounds takes across rounds.)"""
    pts, s, e, root, dear, w1, st1, first, second = _lattice_reference(oracle, n)
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.graph_edges_append(s, e)
        _assert_delta(ctx.graph_cost_update_delta(root), first, "first")
        for i in dear:
            ctx.graph_edges_set_dist(int(i), w1[i:i + 1])
        _assert_delta(ctx.graph_cost_update_delta(root, cap=1), second, "dearer")     # grows from one slot
        assert len(ctx.graph_cost_update_delta(root)[0]) == 0
        _assert_full(ctx, root, st1, "full arrays")


def test_root_change_and_clear(oracle, scene):
    other = 1234
    m = scene.model()
    st_other = _state(m, other)
    with scene.context() as ctx:
        _assert_delta(ctx.graph_cost_update_delta(ROOT), _delta(NOTHING, scene.state0), "first")
        # another root: nothing has been reported for it
        _assert_delta(ctx.graph_cost_update_delta(other), _delta(NOTHING, st_other), "other root")
        assert len(ctx.graph_cost_update_delta(other)[0]) == 0
        # and back: the remembered root is the other one now
        _assert_delta(ctx.graph_cost_update_delta(ROOT), _delta(NOTHING, scene.state0), "back")
        assert len(ctx.graph_cost_update_delta(ROOT)[0]) == 0
        # the mirror is cleared and filled again: the remembered edge ids died with it
        ctx.graph_edges_clear()
        ctx.graph_edges_append(scene.s, scene.e)
        _assert_delta(ctx.graph_cost_update_delta(ROOT), _delta(NOTHING, scene.state0), "after clear")
        _assert_full(ctx, ROOT, scene.state0, "after clear")


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_store_feeds_select_and_target(scene):
    rng = np.random.default_rng(5)
    poses = rng.uniform(-18, 18, (64, 3))
    lmc0, lmc1 = scene.state0[0], scene.state1[0]
    assert not np.array_equal(lmc0, lmc1)

    def both(ctx, lmc):
        return (ctx.find_new_target(poses, 3.0, 40.0, RR, lmc=lmc), ctx.extend_select(poses, R_EDGE, RR, lmc=lmc))
    with scene.context() as ctx:
        want0, want1, const = both(ctx, lmc0), both(ctx, lmc1), both(ctx, np.full(N, 2.5))
        assert any(not np.array_equal(want0[0][k], want1[0][k]) for k in want0[0])       # the two states tell apart
        assert any(not np.array_equal(want0[1][k], const[1][k]) for k in want0[1])
        ctx.graph_cost_update_delta(ROOT, store=True)
        got = both(ctx, None)
        _same(got[0], want0[0], "target, store"); _same(got[1], want0[1], "select, store")
        # store=False leaves the array alone
        ctx.node_cost_set(0, np.full(N, 2.5))
        assert len(ctx.graph_cost_update_delta(ROOT, store=False)[0]) == 0
        ctx.graph_edges_block(scene.blocked)
        _assert_delta(ctx.graph_cost_update_delta(ROOT, store=False), _delta(scene.state0, scene.state1), "no store")
        got = both(ctx, None)
        _same(got[0], const[0], "target, constant"); _same(got[1], const[1], "select, constant")
        # a call that runs out of room has stored all the same
        ctx.graph_edges_unblock(scene.blocked)
        ctx.graph_cost_update_delta(ROOT, store=True)
        ctx.graph_edges_block(scene.blocked)
        rc, needed, *_ = _raw(ctx, ROOT, store=1, cap=0, arrays=False)
        assert rc == _capi.RRTX_E_CAPACITY and needed == len(_delta(scene.state0, scene.state1)[0])
        got = both(ctx, None)
        _same(got[0], want1[0], "target, capacity"); _same(got[1], want1[1], "select, capacity")
