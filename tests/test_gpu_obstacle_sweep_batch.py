"""rrtx_obstacle_sweep_batch: the edge loops of a burst of addNewObstacle calls (R/DRRT_Q.jl:3195-3290 each) in one
pass over the device mirror.  Row j of the CSR is held against the oracle (kdFindWithinRange around obstacle j, then
sweep_edges_batch over the mirror) and against rrtx_obstacle_sweep on the same context, with np.array_equal; block=True
against rrtx_graph_edges_block over the union of the rows, through the cost solve that reads the marks."""
import ctypes as C

import numpy as np
import pytest

from mirror_model import DELTA, RR, Scene
from rrtqx_3d_amd import _capi, drrt

pytestmark = pytest.mark.gpu


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _check(ctx, scene, order, search, cap=None, singles=True):
    """one batched call over positions `order` with ranges `search`: every row against the oracle and the single call"""
    off, ids = ctx.obstacle_sweep_batch(order, search, RR, cap=cap)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and len(off) == len(order) + 1
    rows = _rows_of(off, ids)
    for j, (pos, r) in enumerate(zip(order, search)):
        want = scene.row(pos, r)
        assert np.array_equal(rows[j], want), (j, pos)
        if singles:
            assert np.array_equal(ctx.obstacle_sweep(int(pos), float(r), RR), rows[j]), (j, pos)
    return rows


@pytest.fixture(scope="module")
def scene_a(oracle):
    return Scene(oracle, 3000, 130, inactive=(7,))


def _order_a(scene):
    """all positions shuffled, one listed twice (in two different groups of 64) in place of another"""
    order = np.random.default_rng(1).permutation(scene.K).astype(np.int32)
    drop = [j for j in range(scene.K) if order[j] not in (3, 7, scene.K - 1)][-1]
    order[drop] = order[12]
    return order


def test_scene_a_rows_match_oracle_and_single_sweeps(scene_a):
    """n = 3000, K = 130: 21 000 edges, three groups of obstacles (64, 64, 2)."""
    s = scene_a
    order = _order_a(s)
    search = s.search[order]
    want = [s.row(p, r) for p, r in zip(order, search)]
    # what the scene has to offer, judged on the oracle alone
    total = sum(len(w) for w in want)
    seen = np.bincount(np.concatenate([s.row(p, s.search[p]) for p in range(s.K)]), minlength=len(s.es))
    empty_active = [p for p in range(s.K) if s.active[p] and len(s.row(p, s.search[p])) == 0]
    print(f"scene A: {total} ids, {sum(len(w) == 0 for w in want)} empty rows, {int((seen >= 2).sum())} edges in "
          f"several rows, longest row {max(len(w) for w in want)}")
    assert total >= 500 and len(empty_active) >= 1 and int((seen >= 2).sum()) >= 20
    assert len(s.row(7, s.search[7])) == 0 and len(np.unique(order)) == s.K - 1
    with s.context() as ctx:
        rows = _check(ctx, s, order, search, cap=16)                 # the two-call path
        _check(ctx, s, order, search, cap=total + 7, singles=False)  # ample capacity
        twice = np.nonzero(order == order[12])[0]
        assert len(twice) == 2 and np.array_equal(rows[twice[0]], rows[twice[1]]) and len(rows[twice[0]]) > 0
        for k in (1, 64, 65):                                        # prefixes: one group, a full one, one more
            _check(ctx, s, order[:k], search[:k], singles=False)
        off, ids = ctx.obstacle_sweep_batch([], [], RR)
        assert off.tolist() == [0] and len(ids) == 0
        bad = order.copy()
        bad[100] = s.K
        with pytest.raises(_capi.RrtxError):
            ctx.obstacle_sweep_batch(bad, search, RR)
        with pytest.raises(_capi.RrtxError):
            ctx.obstacle_sweep_batch([-1], [1.0], RR)
        # the root rule, per obstacle: a range that reaches the root exactly, and the next one below it
        d0 = float(np.sqrt(((s.sph[3, :3] - s.pts[0]) ** 2).sum()))
        r_in, r_out = _check(ctx, s, [3, 3], [d0, np.nextafter(d0, 0)])
        assert len(r_in) >= 5 and not np.array_equal(r_in, r_out)    # the root's out-edges are in one and not the other
        # an empty mirror gives empty rows
        ctx.graph_edges_clear()
        off, ids = ctx.obstacle_sweep_batch(order, search, RR)
        assert not off.any() and len(off) == s.K + 1 and len(ids) == 0


def test_scene_b_counts_cross_a_scan_round(oracle):
    """n = 9363, K = 65: 65 541 edges = 64 full blocks of 1024 and 5 edges, two groups (64, 1).  The first group's
    64 x 65 = 4160 per-(obstacle, block) counts are more than a round of the single-workgroup scan takes (4096)."""
    s = Scene(oracle, 9363, 65)
    assert len(s.es) == 64 * 1024 + 5
    order = np.arange(s.K, dtype=np.int32)
    want = [s.row(p, s.search[p]) for p in order]
    total = sum(len(w) for w in want)
    seen = np.bincount(np.concatenate(want), minlength=len(s.es))
    print(f"scene B: {total} ids, {sum(len(w) == 0 for w in want)} empty rows, {int((seen >= 2).sum())} edges in several rows")
    assert 0.01 * len(s.es) <= total <= 0.5 * len(s.es)
    with s.context() as ctx:
        _check(ctx, s, order, s.search, cap=total)                   # exactly enough
        _check(ctx, s, order, s.search, cap=total - 1, singles=False)


def test_block_in_the_call_is_block_over_the_union(scene_a):
    """Both directions of every edge of scene A, root 0.  Solve, sweep 8 obstacles with block=True, update -- against
    solve, 8 single sweeps, rrtx_graph_edges_block(union), update -- against block first, then a full solve."""
    s = scene_a
    es, ee = np.concatenate([s.es, s.ee]), np.concatenate([s.ee, s.es])
    order = np.array([3, 59, 0, 114, 14, 2, 109, 8], dtype=np.int32)       # (59, 114) and (14, 109) share edges
    search = s.search[order]
    want = [s.row(p, r, es, ee) for p, r in zip(order, search)]
    union = np.unique(np.concatenate(want))
    total = sum(len(w) for w in want)
    assert len(union) > 0 and total > len(union)                     # some edge is blocked for two obstacles
    with s.context(es, ee) as c1, s.context(es, ee) as c2, s.context(es, ee) as c3:
        lmc0, par0, _ = c1.graph_cost_to_root(0)
        assert np.isin(par0, union).any()                            # a blocked edge is some node's parent edge
        # a call that fails blocks nothing: one id short of room, block asked for
        off = np.zeros(len(order) + 1, dtype=np.int64)
        ids = np.empty(total, dtype=np.int32)
        needed = C.c_int64()
        rc = c1._lib.rrtx_obstacle_sweep_batch(c1.handle, _capi._ptr(order), len(order), _capi._ptr(search), RR, 1,
                                               _capi._ptr(off), _capi._ptr(ids), total - 1, C.byref(needed))
        assert rc == _capi.RRTX_E_CAPACITY and needed.value == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, lmc0) and np.array_equal(par, par0)
        # 1: blocked by the batched call
        off, ids = c1.obstacle_sweep_batch(order, search, RR, block=True, cap=total)
        for j, row in enumerate(_rows_of(off, ids)):
            assert np.array_equal(row, want[j]), j
        lmc1, par1, _ = c1.graph_cost_update(0)
        # 2: the single calls and one block of the union
        l2, p2, _ = c2.graph_cost_to_root(0)
        assert np.array_equal(l2, lmc0) and np.array_equal(p2, par0)
        got = [c2.obstacle_sweep(int(p), float(r), RR) for p, r in zip(order, search)]
        for j in range(len(order)):
            assert np.array_equal(got[j], want[j]), j
        c2.graph_edges_block(np.unique(np.concatenate(got)))
        lmc2, par2, _ = c2.graph_cost_update(0)
        # 3: blocked before the first solve
        c3.graph_edges_block(union)
        lmc3, par3, _ = c3.graph_cost_to_root(0)
        assert not np.array_equal(lmc3, lmc0)
        for lmc, par in ((lmc1, par1), (lmc2, par2)):
            assert np.array_equal(lmc, lmc3) and np.array_equal(par, par3)
        # blocked edges do not change what a sweep returns
        off, ids = c1.obstacle_sweep_batch(order, search, RR, cap=total)
        assert np.array_equal(ids, np.concatenate(want))


def test_obstacle_sweep_batch_through_the_mirror_names():
    rng = np.random.default_rng(5)
    KD = drrt.KDTree(3)
    S = drrt.CSpace(3, 0.0, [-20] * 3, [20] * 3, [0, 0, 0], [0, 0, 0])
    S.robotRadius, S.delta = RR, DELTA
    S.bind(KD)
    nodes = [drrt.RRTNode(p) for p in rng.uniform(-20, 20, (2000, 3))]
    drrt.kdInsertMany(KD, nodes)
    edges = [drrt.newEdge(nodes[i], nodes[int(j)]) for i in range(2000) for j in rng.integers(0, 2000, 3)]
    assert drrt.registerEdges(KD, edges) == 0
    obs = [drrt.SphereObstacle(c) for c in ([15.0, 15.0, 15.0, 1.0], [1.0, -2.0, 3.0, 4.0], [-6.0, 5.0, 0.0, 2.5],
                                            [3.0, -1.0, 2.0, 3.0])]
    for ob in obs:
        drrt.addObsToCSpace(S, ob)
    picked = [obs[1], obs[3], obs[0], obs[2]]                        # not in list order
    rows = drrt.obstacleSweepBatch(S, KD, picked)
    assert len(rows) == 4 and sum(len(r) for r in rows) > 20
    for ob, row in zip(picked, rows):
        assert np.array_equal(row, drrt.obstacleSweep(S, KD, ob))
    assert drrt.obstacleSweepBatch(S, KD, []) == []
