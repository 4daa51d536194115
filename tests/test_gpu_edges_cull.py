"""rrtx_graph_edges_cull / _compact / _get_culled against tests/cull_model.py (the rule and the renumbering in numpy) and
the oracle's fixed point over the surviving edges (oracle.Graph, reduceInconsistency with hyberBallRad = +Inf; what the
device claims is the order-independent fixed point over the culled graph, not the reference's queue loop with a finite
ball).  Every comparison is exact: np.array_equal on ids and on the 64-bit patterns of costs."""
import ctypes as C

import numpy as np
import pytest

import cull_model as CM
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context
from test_gpu_cost_delta import NOTHING, RR, SPHERE_RADIUS, Scene as DeltaScene, _delta, _lowest_parent
from test_gpu_graph_cost import _oracle_solve

pytestmark = pytest.mark.gpu
INF = float("inf")
N, SEED, BALL_CONSTANT, ROOT = 2000, 5, 30.0, 0
BALL = CM.ball(N, BALL_CONSTANT)
COUNTS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 10239, 10241]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _state(oracle, n, m, root):
    """(rrtLMC, lowest attaining parent edge) of the oracle's fixed point over the model's edges that are not culled,
    parent edges as ids of the model's mirror"""
    keep = np.flatnonzero(m.culled == 0)
    lmc = np.ascontiguousarray(_oracle_solve(oracle, n, m.start[keep], m.end[keep], m.dist[keep], root)[0])
    par = _lowest_parent(lmc, m.start[keep], m.end[keep], m.dist[keep], root)
    return lmc, np.where(par >= 0, keep[np.maximum(par, 0)], -1).astype(np.int32)


class Growth:
    def __init__(self, oracle):
        self.pts, self.s, self.e, self.w = CM.growth_scene(N, SEED, BALL_CONSTANT)
        self.state0 = _state(oracle, N, self.model(), ROOT)
        m = self.model()
        self.ids_all = m.cull(BALL)
        self.state_all = _state(oracle, N, m, ROOT)
        assert np.isin(self.ids_all, self.state0[1]).sum() > 50      # parent edges among the culled (test_cull_scenes.py)

    def model(self):
        return CM.CullModel(self.pts, self.s, self.e)

    def context(self):
        ctx = Context(3)
        ctx.nodes_append(self.pts)
        assert ctx.graph_edges_append(self.s, self.e) == 0
        return ctx


@pytest.fixture(scope="module")
def growth(oracle):
    return Growth(oracle)


def _assert_mirror(ctx, m, what=""):
    assert ctx.n_graph_edges == m.ne, what
    s, e, d, d0 = ctx.graph_edges_get()
    assert np.array_equal(s, m.start) and np.array_equal(e, m.end), what
    assert np.array_equal(_bits(d), _bits(m.dist)) and np.array_equal(_bits(d0), _bits(m.dist0)), what
    assert np.array_equal(ctx.graph_edges_culled(), m.culled), what


def _same_mirror(a, b, what=""):
    assert a.n_graph_edges == b.n_graph_edges, what
    ga, gb = a.graph_edges_get(), b.graph_edges_get()
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]), what
    assert np.array_equal(_bits(ga[2]), _bits(gb[2])) and np.array_equal(_bits(ga[3]), _bits(gb[3])), what


def _set_inf(ctx, ids):
    """rrtx_graph_edges_set_dist(+Inf) for the ids, one call per run of consecutive ids"""
    ids = np.asarray(ids, dtype=np.int64)
    if not len(ids):
        return
    cut = np.flatnonzero(np.diff(ids) != 1) + 1
    for run in np.split(ids, cut):
        ctx.graph_edges_set_dist(int(run[0]), np.full(len(run), INF))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [True, False])
def test_rule_matches_the_model_and_a_set_dist_twin(oracle, growth, subset):
    nodes = np.arange(0, N, 3, dtype=np.int32) if subset else None
    m = growth.model()
    ids = m.cull(BALL, nodes)
    assert len(ids) > 1000
    want = _state(oracle, N, m, ROOT)
    with growth.context() as ctx, growth.context() as twin:
        for c in (ctx, twin):
            first = c.graph_cost_update_delta(ROOT)
            assert np.array_equal(first[0], _delta(NOTHING, growth.state0)[0])
        assert ctx.graph_edges_cull(BALL, nodes) == len(ids)
        _assert_mirror(ctx, m, "after the cull")
        assert ctx.graph_edges_cull(BALL, nodes) == 0                 # idempotent
        _assert_mirror(ctx, m, "after the second cull")
        _set_inf(twin, ids)
        _same_mirror(ctx, twin, "twin")
        assert not twin.graph_edges_culled().any()
        d_ctx, d_twin = ctx.graph_cost_update_delta(ROOT), twin.graph_cost_update_delta(ROOT)
        for a, b in zip(d_ctx[:3], d_twin[:3]):
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                  b.view(np.uint64) if b.dtype == np.float64 else b)
        exp = _delta(growth.state0, want)
        assert len(exp[0]) > 100
        assert np.array_equal(d_ctx[0], exp[0]) and np.array_equal(_bits(d_ctx[1]), _bits(exp[1]))
        assert np.array_equal(d_ctx[2], exp[2])
        lmc, par, _ = ctx.graph_cost_update(ROOT)
        assert np.array_equal(_bits(lmc), _bits(want[0])) and np.array_equal(par, want[1])
        full, _, _ = ctx.graph_cost_to_root(ROOT)                     # and from scratch
        assert np.array_equal(_bits(full), _bits(want[0]))


# ---- 2. threshold and odd costs --------------------------------------------------------------------------------------
def test_threshold_and_odd_costs():
    pts = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.25, 0.0, 0.0], [3.0, 4.25, 0.0], [6.0, 8.0, 0.0], [0.25, 0.25, 0.5]])
    s = np.array([0, 1, 0, 2, 2, 1, 0, 2], dtype=np.int32)
    e = np.array([1, 0, 3, 2, 4, 5, 4, 5], dtype=np.int32)
    for ball, culls_five in ((5.0, False), (np.nextafter(5.0, 0.0), True)):
        m = CM.CullModel(pts, s, e)
        assert m.dist[0] == 5.0
        with Context(3) as ctx:
            ctx.nodes_append(pts)
            ctx.graph_edges_append(s, e)
            m.set_dist(5, [np.nan]); ctx.graph_edges_set_dist(5, [np.nan])       # a NaN cost is kept
            m.block([7]); ctx.graph_edges_block([7])                                 # a blocked short edge is culled
            assert m.dist0[7] < 5.0
            ids = m.cull(ball)
            assert (0 in ids) == culls_five and 7 in ids and 5 not in ids
            assert 1 not in ids and 3 not in ids                                     # start > end, start == end
            assert ctx.graph_edges_cull(ball) == len(ids)
            _assert_mirror(ctx, m, ball)
    # dim 4: the comparison reads the cost set_dist wrote, not the geometry
    p4 = np.array([[0.0, 0.0, 0.0, 0.0], [10.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0]])
    s4, e4 = np.array([0, 0, 1], dtype=np.int32), np.array([1, 2, 2], dtype=np.int32)
    with Context(4) as ctx:
        ctx.nodes_append(p4)
        ctx.graph_edges_append(s4, e4)
        _, _, d, _ = ctx.graph_edges_get()
        assert d.tolist() == [10.0, 0.5, 9.5]
        ctx.graph_edges_set_dist(0, [0.5, 7.0])
        m = CM.CullModel(p4, s4, e4, dist=[0.5, 7.0, 9.5])
        assert m.cull(1.0).tolist() == [1, 2]
        assert ctx.graph_edges_cull(1.0) == 2
        _assert_mirror(ctx, m, "dim 4")


# ---- 3. compaction shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", COUNTS)
def test_compaction_shapes(ne):
    pts = CM.line_nodes()
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        for pattern in CM.PATTERNS:
            s, e, c = CM.line_pattern(ne, pattern)
            m = CM.CullModel(pts, s, e)
            assert ctx.graph_edges_append(s, e) == 0
            assert np.array_equal(m.cull(1.0), np.flatnonzero(c))
            assert ctx.graph_edges_cull(1.0) == int(c.sum()), pattern
            _assert_mirror(ctx, m, pattern)
            want_remap, want_removed = m.compact()
            remap, removed = ctx.graph_edges_compact()
            assert removed == want_removed == int(c.sum()), pattern
            assert remap.dtype == np.int32 and np.array_equal(remap, want_remap), pattern
            assert ctx.n_graph_edges == ne - removed
            _assert_mirror(ctx, m, pattern)                           # the five columns, the culled bytes all zero
            first = ctx.graph_edges_append([3], [0])                  # an append starts at the new count
            assert first == ne - removed and ctx.n_graph_edges == first + 1
            assert ctx.graph_edges_culled(first, 1).tolist() == [0]
            again, none = ctx.graph_edges_compact()                   # nothing culled: the identity
            assert none == 0 and np.array_equal(again, np.arange(first + 1))
            ctx.graph_edges_clear()
            assert ctx.n_graph_edges == 0


def test_pending_touch_of_a_survivor_survives_compaction(oracle):
    """line of 600 nodes rooted at node 0: the parent edges are the initial edges i -> i - 1, the cull takes the current
    edges of length 2, and a cost written to a surviving parent edge between the solve and the compaction -- a touched
    mark still pending -- must reach the update that follows the compaction"""
    n = 600
    pts = CM.line_nodes(n)
    i = np.arange(1, n, dtype=np.int32)
    j = np.arange(0, n - 2, dtype=np.int32)
    s = np.concatenate([i, i - 1, j, j + 2]).astype(np.int32)         # i -> i-1, i-1 -> i, j -> j+2, j+2 -> j
    e = np.concatenate([i - 1, i, j + 2, j]).astype(np.int32)
    order = np.random.default_rng(3).permutation(len(s))              # culled ids all over the mirror
    s, e = s[order], e[order]
    m = CM.CullModel(pts, s, e)
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.graph_edges_append(s, e)
        lmc, par, _ = ctx.graph_cost_to_root(0)
        assert np.array_equal(lmc, np.arange(n, dtype=np.float64))   # a cost is a length: rrtLMC is the node's index
        victim = int(par[300])                                        # a parent edge: start > end, never culled
        assert s[victim] == 300 and e[victim] < 300
        m.set_dist(victim, [0.25]); ctx.graph_edges_set_dist(victim, [0.25])
        ids = m.cull(1.0)
        assert len(ids) == n - 2 and victim not in ids
        assert ctx.graph_edges_cull(1.0) == len(ids)
        want_remap, _ = m.compact()
        remap, removed = ctx.graph_edges_compact()                    # goes through: no culled edge is a parent edge
        assert removed == len(ids) and np.array_equal(remap, want_remap)
        _assert_mirror(ctx, m)
        got, gpar, _ = ctx.graph_cost_update(0)
        want = np.ascontiguousarray(_oracle_solve(oracle, n, m.start, m.end, m.dist, 0)[0])
        assert np.array_equal(_bits(got), _bits(want))
        assert got[300] != lmc[300]                                   # the touched edge took effect
        assert np.array_equal(gpar, _lowest_parent(want, m.start, m.end, m.dist, 0))


# ---- 4. solver state across compaction -------------------------------------------------------------------------------
def _survivor_context(growth, m):
    ctx = Context(3)
    ctx.nodes_append(growth.pts)
    assert ctx.graph_edges_append(m.start, m.end) == 0
    ctx.graph_edges_set_dist(0, m.dist0)
    return ctx


def test_solver_state_is_carried_across_compaction(oracle, growth):
    m = growth.model()
    m.cull(BALL)
    sphere = DeltaScene(oracle).sphere
    rng_ = RR + CM.DELTA + SPHERE_RADIUS
    with growth.context() as ctx:
        ctx.graph_cost_update_delta(ROOT)
        assert ctx.graph_edges_cull(BALL) == len(growth.ids_all)
        d1 = ctx.graph_cost_update_delta(ROOT)
        assert len(d1[0]) > 100
        lmc_b, par_b, _ = ctx.graph_cost_update(ROOT)
        assert np.array_equal(_bits(lmc_b), _bits(growth.state_all[0])) and np.array_equal(par_b, growth.state_all[1])
        want_remap, want_removed = m.compact()
        remap, removed = ctx.graph_edges_compact()
        assert removed == want_removed == len(growth.ids_all) and np.array_equal(remap, want_remap)
        _assert_mirror(ctx, m, "compacted")
        cnt = C.c_int64(-1)
        rc = ctx._lib.rrtx_graph_cost_update_delta(ctx._h, ROOT, 0, None, None, None, 0, C.byref(cnt), None)
        assert rc == _capi.RRTX_OK and cnt.value == 0                 # the next delta reports nothing
        lmc_a, par_a, _ = ctx.graph_cost_update(ROOT)
        assert np.array_equal(_bits(lmc_a), _bits(lmc_b))
        assert np.array_equal(par_a, np.where(par_b >= 0, remap[np.maximum(par_b, 0)], -1))
        with _survivor_context(growth, m) as fresh:
            lmc_f, par_f, _ = fresh.graph_cost_to_root(ROOT)
            assert np.array_equal(_bits(lmc_f), _bits(lmc_a)) and np.array_equal(par_f, par_a)
            for c in (ctx, fresh):
                c.spheres_set(sphere, np.ones(1, dtype=np.uint8))
            rows = [c.obstacle_sweep_batch([0], rng_, RR, block=True) for c in (ctx, fresh)]
            assert len(rows[0][1]) > 0
            assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
            rows = [c.obstacle_release_batch([0], rng_, RR, unblock=True) for c in (ctx, fresh)]
            assert len(rows[0][1]) > 0
            assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
            _same_mirror(ctx, fresh, "after sweep and release")
            la, pa, _ = ctx.graph_cost_update(ROOT)
            lf, pf, _ = fresh.graph_cost_update(ROOT)
            assert np.array_equal(_bits(la), _bits(lf)) and np.array_equal(pa, pf)


def test_compact_straight_after_a_cull_is_refused(growth):
    m = growth.model()
    m.cull(BALL)
    with growth.context() as ctx:
        ctx.graph_cost_update_delta(ROOT)
        ctx.graph_edges_cull(BALL)
        with pytest.raises(RrtxError) as err:
            ctx.graph_edges_compact()
        assert err.value.code == _capi.RRTX_E_STATE and "rrtx_graph_cost_update" in str(err.value)
        _assert_mirror(ctx, m, "refused: nothing changed")
        ctx.graph_cost_update(ROOT)
        remap, removed = ctx.graph_edges_compact()                    # after the update it goes through
        assert removed == len(growth.ids_all)
    with growth.context() as ctx:                                     # no kept solve: always through
        ctx.graph_edges_cull(BALL)
        assert ctx.graph_edges_compact()[1] == len(growth.ids_all)
        m.compact()
        _assert_mirror(ctx, m, "no solve")


def test_delta_after_compaction_reports_what_differs(growth):
    """graph_cost_update, not the delta, between the cull and the compaction: the baseline is still the state before the
    cull, renumbered; the next delta reports exactly the nodes whose cost or parent edge differ"""
    m = growth.model()
    m.cull(BALL)
    with growth.context() as ctx:
        ctx.graph_cost_update_delta(ROOT)
        ctx.graph_edges_cull(BALL)
        ctx.graph_cost_update(ROOT)
        remap, _ = ctx.graph_edges_compact()
        node, lmc, par, _ = ctx.graph_cost_update_delta(ROOT)
        exp = _delta(growth.state0, growth.state_all)                 # in the ids before the compaction
        assert np.array_equal(node, exp[0]) and np.array_equal(_bits(lmc), _bits(exp[1]))
        assert np.array_equal(par, np.where(exp[2] >= 0, remap[np.maximum(exp[2], 0)], -1))
        assert (growth.state0[1][exp[0]] != growth.state_all[1][exp[0]]).any()
        assert len(ctx.graph_cost_update_delta(ROOT)[0]) == 0


def test_compaction_between_an_append_and_the_next_solve(oracle, growth):
    """The kept solve has not seen the last edges of the mirror when it is compacted: solve the tree of its first 1 500
    nodes, cull at that tree's ball, update; then the edges of the other 500 nodes arrive, and a second cull at the
    final ball takes edges on both sides of the mark -- edges the solve knows and edges it has never seen -- of start
    nodes chosen so that no parent edge is among them; compact with no solve in between; then graph_cost_update, which
    has to take exactly the edges behind the renumbered mark for new.  Against the oracle and a fresh context of the
    survivors, bit for bit."""
    n1 = 1500
    cut = int(np.searchsorted(np.maximum(growth.s, growth.e), n1))         # edges are in the order of their later node
    assert np.all(np.maximum(growth.s, growth.e)[:cut] < n1) and np.all(np.maximum(growth.s, growth.e)[cut:] >= n1)
    ball1 = CM.ball(n1, BALL_CONSTANT)
    m = CM.CullModel(growth.pts, growth.s[:cut], growth.e[:cut])
    with growth.context() as probe:                                         # (the helper appends every edge: start over)
        probe.graph_edges_clear()
        ctx = probe
        assert ctx.graph_edges_append(growth.s[:cut], growth.e[:cut]) == 0
        ctx.graph_cost_update_delta(ROOT)
        assert ctx.graph_edges_cull(ball1) == len(m.cull(ball1)) > 0
        lmc1, par1, _ = ctx.graph_cost_update(ROOT)
        want1 = _state(oracle, N, m, ROOT)
        assert np.array_equal(_bits(lmc1), _bits(want1[0])) and np.array_equal(par1, want1[1])
        assert np.isinf(lmc1[n1:]).all()
        # the rest of the tree arrives; no solve from here to the compaction
        assert ctx.graph_edges_append(growth.s[cut:], growth.e[cut:]) == cut
        m.append(growth.s[cut:], growth.e[cut:])
        cand = m.would_cull(BALL)
        is_parent = np.isin(cand, par1[par1 >= 0])
        assert is_parent.any()                                              # the whole cull would be refused
        nodes = np.setdiff1d(np.unique(m.start[cand]), m.start[cand[is_parent]]).astype(np.int32)
        ids = m.cull(BALL, nodes)
        assert (ids < cut).sum() > 50 and (ids >= cut).sum() > 50           # culled ids before and behind the mark
        assert not np.isin(ids, par1[par1 >= 0]).any()
        assert ctx.graph_edges_cull(BALL, nodes) == len(ids)
        _assert_mirror(ctx, m, "second cull")
        want_remap, want_removed = m.compact()
        remap, removed = ctx.graph_edges_compact()
        assert removed == want_removed and np.array_equal(remap, want_remap)
        _assert_mirror(ctx, m, "compacted")
        lmc2, par2, _ = ctx.graph_cost_update(ROOT)
        want2 = _state(oracle, N, m, ROOT)
        assert np.isfinite(want2[0][n1:]).any() and (want2[0][:n1] < lmc1[:n1]).any()   # new nodes reached, old ones lowered
        assert np.array_equal(_bits(lmc2), _bits(want2[0])) and np.array_equal(par2, want2[1])
        with _survivor_context(growth, m) as fresh:
            lmc_f, par_f, _ = fresh.graph_cost_to_root(ROOT)
            assert np.array_equal(_bits(lmc_f), _bits(lmc2)) and np.array_equal(par_f, par2)
        # and the delta after it: against the baseline of the first report, renumbered
        node, lmc, par, _ = ctx.graph_cost_update_delta(ROOT)
        base = _state(oracle, N, CM.CullModel(growth.pts, growth.s[:cut], growth.e[:cut]), ROOT)
        base_par = np.where(base[1] >= 0, remap[np.maximum(base[1], 0)], -1)
        base_par = np.where((base[1] >= 0) & (base_par < 0), -2, base_par).astype(np.int32)   # a removed edge: no id equals it
        exp = _delta((base[0], base_par), want2)
        assert np.array_equal(node, exp[0]) and np.array_equal(_bits(lmc), _bits(exp[1])) and np.array_equal(par, exp[2])


# ---- 5. errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_mirror_untouched(growth):
    m = growth.model()
    with growth.context() as ctx:
        lib, h = ctx._lib, ctx._h
        cnt = C.c_int64(-7)
        ok = np.array([1, 2], dtype=np.int32)
        for ball, nodes, k in ((float("nan"), None, 0), (-1.0, None, 0), (1.0, ok, -1), (1.0, None, 2),
                               (1.0, np.array([1, N], dtype=np.int32), 2), (1.0, np.array([-1, 1], dtype=np.int32), 2)):
            assert lib.rrtx_graph_edges_cull(h, ball, _capi._ptr(nodes), k, C.byref(cnt)) == _capi.RRTX_E_INVALID, (ball, k)
            assert cnt.value == 0
        _assert_mirror(ctx, m, "invalid culls")
        assert lib.rrtx_graph_edges_cull(h, 1.0, _capi._ptr(ok), 0, C.byref(cnt)) == _capi.RRTX_OK and cnt.value == 0
        assert ctx.graph_edges_cull(1.0, []) == 0
        assert ctx.graph_edges_cull(INF) == 0                         # nothing is beyond an infinite ball
        assert lib.rrtx_graph_edges_cull(h, 1.0, _capi._ptr(ok), 2, None) == _capi.RRTX_OK      # n_culled may be NULL
        m.cull(1.0, ok)
        _assert_mirror(ctx, m, "two nodes")
        short = np.zeros(m.ne - 1, dtype=np.int32)
        assert lib.rrtx_graph_edges_compact(h, _capi._ptr(short), m.ne - 1, C.byref(cnt)) == _capi.RRTX_E_CAPACITY
        assert cnt.value == 0
        _assert_mirror(ctx, m, "short remap")
        out = np.zeros(4, dtype=np.uint8)
        for first, n in ((-1, 2), (m.ne - 1, 2), (0, -1), (m.ne + 1, 0)):
            assert lib.rrtx_graph_edges_get_culled(h, first, n, _capi._ptr(out)) == _capi.RRTX_E_INVALID
        assert lib.rrtx_graph_edges_get_culled(h, 0, 2, None) == _capi.RRTX_E_INVALID
        assert lib.rrtx_graph_edges_compact(h, None, 0, None) == _capi.RRTX_OK                   # remap and n_removed NULL
        m.compact()
        _assert_mirror(ctx, m, "compacted without a remap")
        # clear after a cull: the flags go with the mirror
        assert ctx.graph_edges_cull(BALL) > 0
        ctx.graph_edges_clear()
        assert ctx.graph_edges_append(growth.s, growth.e) == 0
        _assert_mirror(ctx, growth.model(), "after clear")
    with Context(3) as empty:                                         # the empty mirror
        empty.nodes_append(growth.pts[:4])
        assert empty.graph_edges_cull(1.0) == 0 and empty.graph_edges_cull(1.0, [0, 3]) == 0
        remap, removed = empty.graph_edges_compact()
        assert removed == 0 and len(remap) == 0 and len(empty.graph_edges_culled()) == 0
