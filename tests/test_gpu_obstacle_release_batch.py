"""rrtx_obstacle_release_batch: the edge loops of a burst of corrected removeObstacle calls (R/DRRT_Q.jl:3295-3362 each)
in one pass over the device mirror, and rrtx_graph_edges_unblock (edge.dist = edge.distOriginal, :3342).  Row j of the
CSR is held against the oracle alone, called once per row (kdFindWithinRange around obstacle j, then sweep_edges_batch
with remove=True over the mirror, the staying spheres and obstacle j in use), with np.array_equal; unblock=True against
rrtx_graph_edges_unblock over the union of the rows, through the cost solve that reads the marks."""
import ctypes as C

import numpy as np
import pytest

from mirror_model import DELTA, RR, Scene
from rrtqx_3d_amd import _capi, drrt

pytestmark = pytest.mark.gpu


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _check(ctx, scene, leaving, search, dist_host, cap=None):
    """one release of positions `leaving` with ranges `search`: every row against the oracle"""
    off, ids = ctx.obstacle_release_batch(leaving, search, RR, cap=cap)
    assert off.dtype == np.int64 and ids.dtype == np.int32 and len(off) == len(leaving) + 1
    rows = _rows_of(off, ids)
    for j, (pos, r) in enumerate(zip(leaving, search)):
        assert np.array_equal(rows[j], scene.release_row(leaving, pos, r, dist_host)), (j, pos)
    return rows


LEAVING_A = np.array(list(range(0, 100, 2)) + [7, 101, 129] + list(range(1, 30, 2)), dtype=np.int32)


class SceneA(Scene):
    """n = 3000, K = 130: 21 000 edges.  Flags all 1 except position 7; blocked: the batched sweep of positions 0..99
    and 50 ids by hand that no sweep returned; 68 positions leave, in two groups (64, 4), position 7 twice."""

    def __init__(self, oracle):
        super().__init__(oracle, 3000, 130, inactive=(7,))
        ne = len(self.es)
        sweeps = [self.sweep_row(p, self.search[p]) if self.active[p] else np.zeros(0, np.int32) for p in range(100)]
        self.union = np.unique(np.concatenate(sweeps))
        self.hand = np.setdiff1d(np.arange(0, ne, 97), self.union)[:50].astype(np.int32)
        self.blocked = np.union1d(self.union, self.hand).astype(np.int32)
        self.dist_host = np.ones(ne)
        self.dist_host[self.blocked] = np.inf
        self.leaving = LEAVING_A
        self.lsearch = self.search[self.leaving]

    def blocked_context(self):
        ctx = self.context()
        off, ids = ctx.obstacle_sweep_batch(np.arange(100, dtype=np.int32), self.search[:100], RR, block=True)
        assert np.array_equal(np.unique(ids), self.union)
        ctx.graph_edges_block(self.hand)
        return ctx


@pytest.fixture(scope="module")
def scene_a(oracle):
    return SceneA(oracle)


def test_scene_a_offers_what_the_checks_need(scene_a):
    """Judged on the oracle alone, before the device is touched.  Counts of this scene: 920 ids in all rows, 896
    distinct, 24 edges in several rows, 14 empty rows, 149 blocked edges that hit a leaving obstacle and are kept by a
    staying one, 43 edges that hit a leaving obstacle (position 7 included) and are not blocked, 0 of the 50 hand-blocked
    ids, 4 edges that start at the root (ids 0..6) in some row."""
    s = scene_a
    assert len(s.es) == 21000 and len(s.hand) == 50 and len(s.leaving) == 68 and len(np.unique(s.leaving)) == 67
    want = [s.release_row(s.leaving, p, r, s.dist_host) for p, r in zip(s.leaving, s.lsearch)]
    hits = [s.sweep_row(p, r) for p, r in zip(s.leaving, s.lsearch)]          # in range and colliding, blocked or not
    allw = np.concatenate(want)
    seen = np.bincount(allw, minlength=len(s.es))
    kept = np.unique(np.concatenate([np.setdiff1d(np.intersect1d(h, s.blocked), w) for h, w in zip(hits, want)]))
    unblocked = np.setdiff1d(np.unique(np.concatenate(hits)), s.blocked)
    root_out = np.intersect1d(np.flatnonzero(s.es == 0), allw)
    print(f"scene A: {len(allw)} ids in all rows, {int((seen >= 1).sum())} distinct, {int((seen >= 2).sum())} edges in "
          f"several rows, {sum(len(w) == 0 for w in want)} empty rows, {len(kept)} kept by a staying sphere, "
          f"{len(unblocked)} hit but not blocked, {int(np.isin(s.hand, allw).sum())} hand-blocked ids returned, "
          f"{len(root_out)} out-edges of the root")
    assert len(allw) >= 500 and int((seen >= 2).sum()) >= 10 and sum(len(w) == 0 for w in want) >= 1
    assert len(kept) >= 50 and len(unblocked) >= 10 and int(np.isin(s.hand, allw).sum()) == 0 and len(root_out) >= 1


def test_scene_a_rows_match_the_oracle(scene_a):
    s = scene_a
    L, search = s.leaving, s.lsearch
    total = sum(len(s.release_row(L, p, r, s.dist_host)) for p, r in zip(L, search))
    with s.blocked_context() as ctx:
        rows = _check(ctx, s, L, search, s.dist_host, cap=16)                # the two-call path
        _check(ctx, s, L, search, s.dist_host, cap=total + 7)                # ample capacity
        # against the existing entry points on the same context, for the leaving obstacles that are in use
        stay = s.stay(L)
        for j, (pos, r) in enumerate(zip(L, search)):
            if not s.active[pos]:
                continue
            ids = ctx.obstacle_sweep(int(pos), float(r), RR)
            ids = ids[np.isin(ids, s.blocked)]
            if len(ids):
                hit, _ = ctx.edges_check_idx(s.es[ids], s.ee[ids], RR, obstacle=-1, obstacle_mask=stay, want_first=False)
                ids = ids[hit == 0]
            assert np.array_equal(rows[j], ids), (j, pos)
        # the leaving obstacle's own flag is not read
        flags = s.active.copy()
        flags[L[::2]] = 0
        ctx.spheres_set(s.sph, flags)
        for a, b in zip(rows, _rows_of(*ctx.obstacle_release_batch(L, search, RR))):
            assert np.array_equal(a, b)
        ctx.spheres_set(s.sph, s.active)
        for k in (1, 64, 65):                                                # prefixes: one group, a full one, one more
            _check(ctx, s, L[:k], search[:k], s.dist_host)
        off, ids = ctx.obstacle_release_batch([], [], RR)
        assert off.tolist() == [0] and len(ids) == 0
        # a position listed twice
        p = int(L[[j for j in range(len(L)) if len(rows[j]) > 0][0]])
        r2 = _check(ctx, s, np.array([p, p], dtype=np.int32), s.search[[p, p]], s.dist_host)
        assert np.array_equal(r2[0], r2[1]) and len(r2[0]) > 0
        bad = L.copy()
        bad[66] = s.K
        with pytest.raises(_capi.RrtxError):
            ctx.obstacle_release_batch(bad, search, RR)
        with pytest.raises(_capi.RrtxError):
            ctx.obstacle_release_batch([-1], [1.0], RR)
        for a, b in zip(rows, _rows_of(*ctx.obstacle_release_batch(L, search, RR))):     # a refused call changed nothing
            assert np.array_equal(a, b)
        # after graph_edges_clear every row is empty
        ctx.graph_edges_clear()
        off, ids = ctx.obstacle_release_batch(L, search, RR)
        assert not off.any() and len(off) == len(L) + 1 and len(ids) == 0
    # nothing blocked: every row is empty
    with s.context() as ctx:
        off, ids = ctx.obstacle_release_batch(L, search, RR)
        assert not off.any() and len(off) == len(L) + 1 and len(ids) == 0


def test_root_rule_is_per_obstacle(scene_a):
    """Only the root's out-edges are blocked; sphere 3 sits 2.0 from the root.  A range that reaches the root exactly
    takes it (<=), the next double below does not."""
    s = scene_a
    root_out = np.flatnonzero(s.es == 0).astype(np.int32)
    dist = np.ones(len(s.es))
    dist[root_out] = np.inf
    d0 = float(np.sqrt(((s.sph[3, :3] - s.pts[0]) ** 2).sum()))
    L, search = np.array([3, 3], dtype=np.int32), np.array([d0, np.nextafter(d0, 0)])
    w_in, w_out = (s.release_row(L, 3, r, dist) for r in search)
    assert len(w_in) >= 1 and np.isin(w_in, root_out).all() and not np.array_equal(w_in, w_out)
    with s.context() as ctx:
        ctx.graph_edges_block(root_out)
        r_in, r_out = _check(ctx, s, L, search, dist)
        assert not np.array_equal(r_in, r_out)


def test_counts_cross_a_scan_round(oracle):
    """n = 9363, K = 65: 65 541 edges = 64 full blocks of 1024 and 5 edges, two groups (64, 1); the first group's
    64 x 65 = 4160 per-(obstacle, block) counts are more than a round of the single-workgroup scan takes.  Everything
    the batched sweep of all 65 returns is blocked, then all 65 leave.  Seed n + K as generated; position 64 is the
    generator's tiny sphere in a corner and its row is empty, so the 65 positions leave in the order 64, 0, 1, ..., 63:
    the second group is position 63, whose row the oracle finds non-empty."""
    s = Scene(oracle, 9363, 65)
    assert len(s.es) == 64 * 1024 + 5
    L = np.roll(np.arange(s.K, dtype=np.int32), 1)
    search = s.search[L]
    dist = np.ones(len(s.es))
    dist[np.unique(np.concatenate([s.sweep_row(p, s.search[p]) for p in range(s.K)]))] = np.inf
    want = [s.release_row(L, p, r, dist) for p, r in zip(L, search)]
    total = sum(len(w) for w in want)
    print(f"counts scene: {total} ids, {sum(len(w) == 0 for w in want)} empty rows")
    assert any(len(w) > 0 for w in want[:64]) and len(want[64]) > 0
    with s.context() as ctx:
        ctx.obstacle_sweep_batch(np.arange(s.K, dtype=np.int32), s.search, RR, block=True)
        _check(ctx, s, L, search, dist, cap=total)                           # exactly enough
        _check(ctx, s, L, search, dist, cap=total - 1)


def test_release_of_everything_blocked_is_the_sweep(oracle):
    """The seam of the head the two passes over the mirror share.  n = 300, K = 66, every flag 1: 2 100 edges = two
    full blocks of 1024 and 52 edges, two groups of obstacles (64, 2).  With every edge of the mirror blocked and all 66
    spheres leaving, no sphere stays, so the release's row j is the sweep's row j.  Seed n + K as generated: the oracle
    finds 15 non-empty rows in the first group and position 64 (14 ids) in the second; position 65 is the tiny sphere."""
    s = Scene(oracle, 300, 66)
    assert len(s.es) == 2 * 1024 + 52 and s.active.all()
    L = np.arange(s.K, dtype=np.int32)
    want = [s.row(p, s.search[p]) for p in L]
    assert any(len(w) > 0 for w in want[:64]) and any(len(w) > 0 for w in want[64:])
    dist = np.full(len(s.es), np.inf)
    with s.context() as ctx:
        swept = _rows_of(*ctx.obstacle_sweep_batch(L, s.search, RR))
        ctx.graph_edges_block(np.arange(len(s.es), dtype=np.int32))
        freed = _check(ctx, s, L, s.search, dist)                            # every row against the oracle's release
        for j in range(s.K):
            assert np.array_equal(freed[j], swept[j]), j
            assert np.array_equal(swept[j], want[j]), j


def test_unblock_in_the_call_is_unblock_over_the_union(scene_a):
    """Both directions of every edge of scene A, root 0.  Solve, block 8 obstacles' sweeps, update, release 4 of them
    with unblock=True, update -- against the same with rrtx_graph_edges_unblock(union) -- against a mirror where only
    what stays blocked was ever blocked, solved in full."""
    s = scene_a
    es, ee = np.concatenate([s.es, s.ee]), np.concatenate([s.ee, s.es])
    order = np.array([3, 59, 0, 114, 14, 2, 109, 8], dtype=np.int32)
    L = order[:4]
    search, lsearch = s.search[order], s.search[L]
    swept = np.unique(np.concatenate([s.sweep_row(p, r, es, ee) for p, r in zip(order, search)]))
    dist = np.ones(len(es))
    dist[swept] = np.inf
    want = [s.release_row(L, p, r, dist, es, ee) for p, r in zip(L, lsearch)]
    freed = np.unique(np.concatenate(want))
    total = sum(len(w) for w in want)
    assert 0 < len(freed) < len(swept) and total >= 1
    with s.context(es, ee) as c1, s.context(es, ee) as c2, s.context(es, ee) as c3:
        lmc0, par0, _ = c1.graph_cost_to_root(0)
        c1.obstacle_sweep_batch(order, search, RR, block=True)
        lmc_b, par_b, _ = c1.graph_cost_update(0)
        assert not np.array_equal(lmc_b, lmc0)
        # a call that fails unblocks nothing: one id short of room, unblock asked for
        off = np.zeros(len(L) + 1, dtype=np.int64)
        ids = np.empty(total, dtype=np.int32)
        needed = C.c_int64()
        rc = c1._lib.rrtx_obstacle_release_batch(c1.handle, _capi._ptr(L), len(L), _capi._ptr(lsearch), RR, 1,
                                                 _capi._ptr(off), _capi._ptr(ids), total - 1, C.byref(needed))
        assert rc == _capi.RRTX_E_CAPACITY and needed.value == total
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, lmc_b) and np.array_equal(par, par_b)
        # 1: unblocked by the batched call
        off, ids = c1.obstacle_release_batch(L, lsearch, RR, unblock=True, cap=total)
        for j, row in enumerate(_rows_of(off, ids)):
            assert np.array_equal(row, want[j]), j
        lmc1, par1, _ = c1.graph_cost_update(0)
        # 2: the release without unblock, then one unblock of the union
        c2.graph_cost_to_root(0)
        c2.obstacle_sweep_batch(order, search, RR, block=True)
        l2, p2, _ = c2.graph_cost_update(0)
        assert np.array_equal(l2, lmc_b) and np.array_equal(p2, par_b)
        off, ids = c2.obstacle_release_batch(L, lsearch, RR, unblock=False)
        assert np.array_equal(ids, np.concatenate(want))
        l2, p2, _ = c2.graph_cost_update(0)
        assert np.array_equal(l2, lmc_b) and np.array_equal(p2, par_b)      # unblock=False wrote nothing
        c2.graph_edges_unblock(np.unique(ids))
        lmc2, par2, _ = c2.graph_cost_update(0)
        # 3: only what stays blocked, before the first solve
        c3.graph_edges_block(np.setdiff1d(swept, freed))
        lmc3, par3, _ = c3.graph_cost_to_root(0)
        for lmc, par in ((lmc1, par1), (lmc2, par2)):
            assert np.array_equal(lmc, lmc3) and np.array_equal(par, par3)
        assert not np.array_equal(lmc3, lmc_b)
        # released edges are no longer blocked: a second release finds none of them
        off, ids = c1.obstacle_release_batch(L, lsearch, RR)
        assert len(ids) == 0


def test_unblock_restores_what_set_dist_wrote(scene_a):
    """distOriginal follows rrtx_graph_edges_set_dist: set 100 costs, block the ids, unblock them, update -- equal to a
    context that set the costs and never blocked."""
    s = scene_a
    es, ee = np.concatenate([s.es, s.ee]), np.concatenate([s.ee, s.es])
    first = len(s.es)                                                       # the edges into the root come first here
    vals = np.random.default_rng(11).uniform(0.25, 3.0, 100)
    ids = np.arange(first, first + 100, dtype=np.int32)
    with s.context(es, ee) as c1, s.context(es, ee) as c2:
        lmc0, _, _ = c1.graph_cost_to_root(0)
        c1.graph_edges_set_dist(first, vals)
        c1.graph_edges_block(ids)
        lmc_b, _, _ = c1.graph_cost_update(0)
        c1.graph_edges_unblock(ids)
        c1.graph_edges_unblock(ids[:0])                                      # n == 0
        lmc1, par1, _ = c1.graph_cost_update(0)
        c2.graph_edges_set_dist(first, vals)
        lmc2, par2, _ = c2.graph_cost_to_root(0)
        assert np.array_equal(lmc1, lmc2) and np.array_equal(par1, par2)
        assert not np.array_equal(lmc1, lmc0) and not np.array_equal(lmc1, lmc_b)
        # an id outside the mirror: refused, nothing written
        with pytest.raises(_capi.RrtxError):
            c1.graph_edges_unblock(np.array([0, len(es)], dtype=np.int32))
        with pytest.raises(_capi.RrtxError):
            c1.graph_edges_unblock(np.array([-1], dtype=np.int32))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, lmc2) and np.array_equal(par, par2)
        # an id that is not blocked is rewritten with its own value
        c1.graph_edges_unblock(np.arange(0, 300, dtype=np.int32))
        lmc, par, _ = c1.graph_cost_update(0)
        assert np.array_equal(lmc, lmc2) and np.array_equal(par, par2)


def test_obstacle_release_batch_through_the_mirror_names():
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
    swept = drrt.obstacleSweepBatch(S, KD, obs, block=True)
    picked = [obs[3], obs[0], obs[2]]                                # not in list order; obs[1] stays
    rows = drrt.obstacleReleaseBatch(S, KD, picked)
    assert len(rows) == 3 and 0 < sum(len(r) for r in rows) < sum(len(r) for r in swept)
    off, ids = KD.ctx.obstacle_release_batch([drrt._list_position(S, ob) for ob in picked],
                                             [RR + DELTA + ob.radius for ob in picked], RR)
    for j, row in enumerate(rows):
        assert np.array_equal(row, ids[off[j]:off[j + 1]])
    drrt.unblockEdges(KD, np.unique(np.concatenate(rows)))
    assert sum(len(r) for r in drrt.obstacleReleaseBatch(S, KD, picked)) == 0
    assert drrt.obstacleReleaseBatch(S, KD, []) == []
