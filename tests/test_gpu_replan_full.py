"""The replanning half of the hot path at full size against the batched CPU oracle: the obstacle sweeps
(rrtx_obstacle_sweep, rrtx_obstacle_sweep_polygon add / remove), the edge blocking (rrtx_graph_edges_block,
rrtx_graph_edges_set_dist) and the cost propagation (rrtx_graph_cost_to_root, rrtx_graph_cost_update).

Sizes are chosen so that the device paths which only switch on at full size run: more than 2^20 mirrored edges
(more than one 4096-counter round of the block-count scan), a sweep with more than 2^21 candidates (later chunks of the Dubins
check through edge ids), more than 2^21 nodes (1024 tiles of 2048 nodes in the tile-sum scan), appended edges on both
sides of the in-edge CSR rebuild threshold, and nodes appended past the last solve's buffers.

Every comparison is exact: edge ids with np.array_equal, rrtLMC bit for bit.  Parent edges are held to the lowest
attaining edge id on every node (test_gpu_graph_cost._check_parents) and to the oracle's parent wherever one edge
alone attains the minimum; no more than 1 % of the finite non-root nodes may have a tie (asserted on the oracle's
solution), which caps what the second comparison leaves out.  Each step prints one "REPLAN {...}" line: counts,
oracle and device seconds."""
import json
import math
import time

import numpy as np
import pytest

from rrtqx_3d_amd import synth
from rrtqx_3d_amd.context import Context
from test_gpu_graph_cost import _check_parents, _edge_dist

pytestmark = pytest.mark.gpu
INF = float("inf")
RR, DELTA = 0.5, 8.0
TAIL_BASE = 262144                 # graph_cost_impl rebuilds the in-edge CSR inside an update once tail > this + E0 / 8
SCAN_BLOCKS = 1024 * 1024          # (one lane of the former block-count scan per block of 1024 edges up to this many edges)
DUB_CHUNK = 1 << 21                # launch_dubins_edges_idx / the steering kernel: edges per chunk
SCAN_TILES = 1024 * 2048           # (one lane of the former tile-sum scan per tile of 2048 nodes up to this many nodes)


def _report(step, **kv):
    print("REPLAN " + json.dumps(dict(step=step, **kv), default=float), flush=True)


class _Clock:
    def __init__(self):
        self.t = {}

    def __call__(self, name):
        clock = self

        class _Span:
            def __enter__(self):
                self.t0 = time.perf_counter()

            def __exit__(self, *exc):
                clock.t[name] = clock.t.get(name, 0.0) + time.perf_counter() - self.t0
        return _Span()

    def seconds(self):
        return {k: float(f"{v:.4g}") for k, v in self.t.items()}


def _solve(oracle, n, s, e, w, root):
    """a fresh oracle graph at the fixed point (node n: a goal that stays at Inf, so the queue runs dry)"""
    g = oracle.Graph(n + 1)                       # every node starts at rrtLMC = rrtTreeCost = Inf
    assert g.add_edges(s, e, w) == 0
    g.set_node(root, 0.0, INF)
    g.verifyInQueue(root)
    g.reduceInconsistency(n, root)
    return g


def _reference_block(oracle_graph, n, root, ids):
    """the reference's own sequence after an obstacle appears: blockEdge per id, propogateDescendants,
    reduceInconsistency"""
    oracle_graph.block_edges(ids)
    oracle_graph.propogateDescendants()
    oracle_graph.reduceInconsistency(n, root)


def _compare(lmc, par, g, s, e, w, root, label):
    """device (lmc, par) against oracle graph g on the graph (s, e, w); returns the counts compared"""
    n = len(lmc)
    want, want_par = g.lmc()[:n], g.parent_edge()[:n]
    assert len(s) == len(e) == len(w) and len(want) == n
    assert np.array_equal(lmc, want), (label, _first_diff(lmc, want))
    att = _check_parents(lmc, par, s, e, w, root)         # lmc == the oracle's: these are the oracle's attaining edges
    n_att = np.bincount(s[att], minlength=n)
    fin = np.isfinite(want)
    fin[root] = False
    ties = int((n_att[fin] >= 2).sum())
    assert ties <= 0.01 * fin.sum(), (label, ties, int(fin.sum()))
    single = n_att == 1
    assert np.array_equal(par[single], want_par[single]), label
    return dict(nodes=n, edges=len(s), reachable=int(fin.sum()) + 1, ties=ties, parents_vs_oracle=int(single.sum()))


def _first_diff(a, b):
    bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
    if not bad.size:
        return None
    i = int(bad[0])
    return dict(node=i, device=float(a[i]), oracle=float(b[i]), differ=int(bad.size))


def _mask(n, idx):
    m = np.zeros(n, dtype=np.uint8)
    m[np.asarray(idx, dtype=np.int64)] = 1
    return m


def _runs(ids):
    """contiguous runs of sorted ids"""
    ids = np.sort(np.asarray(ids, dtype=np.int64))
    return np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1) if ids.size else []


def _mirror(ctx, oracle, trees, q_first, Q, r, n_check=512):
    """both directed edges of every pair within r, per node in ascending order, own node excluded: the rows Q are
    nodes q_first.. of the tree; with q_first > 0 only the pairs with an older node (or an earlier row of Q) are new.

    The lists come from the device's range search (as bench.py builds its mirror); n_check of them, spread over Q, are
    held bit for bit to oracle.range_batch on the same tree.  All of them from the oracle would take a quarter of an
    hour on 16 threads at 500 k nodes: kdFindWithinRange as the reference writes it prunes a subtree on one side of
    the split only, some 30 ms per search at this size.  Every check after this one runs on the same edge list in
    both, so the sweeps and costs are held to the oracle whatever the lists."""
    off_l, idx_l = [np.zeros(1, dtype=np.int64)], []
    for a in range(0, len(Q), 32768):
        b = min(len(Q), a + 32768)
        off, idx, _ = ctx.nn_radius(Q[a:b], r, cap=64 * (b - a))
        off_l.append(off[1:] + off_l[-1][-1])
        idx_l.append(idx)
    dev = dict(offsets=np.concatenate(off_l), idx=np.concatenate(idx_l))
    pick = np.unique(np.r_[0, len(Q) - 1, np.random.default_rng(len(Q)).choice(len(Q), min(n_check, len(Q)),
                                                                             replace=False)])
    ref = oracle.range_batch(trees, Q[pick], r, per_sample=32.0, nearest=False)
    oracle.assert_same_results(oracle.take_samples(dev, pick), ref, ("offsets", "idx"), names=pick + q_first,
                               label="mirror range lists: ")
    own = np.repeat(np.arange(q_first, q_first + len(Q), dtype=np.int32), np.diff(dev["offsets"]))
    nb = dev["idx"]
    if q_first == 0:
        keep = own != nb
        return own[keep], nb[keep]
    keep = nb < own
    return np.concatenate([own[keep], nb[keep]]), np.concatenate([nb[keep], own[keep]])


def _dubins_time_costs(oracle, pts, s, e, r_min):
    """(edge.dist of a DubinsEdge with time, the mirror's cost: the same with Inf where start.t <= end.t -- planning
    runs in reverse time)"""
    d = np.empty(len(s))
    for a in range(0, len(s), DUB_CHUNK):
        b = min(len(s), a + DUB_CHUNK)
        d[a:b] = oracle.dubins_edges_batch(pts[s[a:b]], pts[e[a:b]], r_min, has_time=True, piecewise=True)["cost"]
    return d, np.where(pts[s, 2] > pts[e, 2], d, INF)


def test_c5_replanning_cycle(oracle):
    """BASELINE config 5's scene as bench.py --config C5 builds it (restated): DubinsEdge with time, 500 k nodes,
    256 polygons of which the moving ones not yet seen are inactive, the mirror of every pair within 2.0.  The full
    solve, four cycles of an appearing obstacle, two growths of the tree and two removals."""
    t_start = time.perf_counter()
    N, M, B, CYCLES = 500_000, 256, 16384, 4
    r_min, rr, delta, r_graph = synth.R_MIN_TIME, 0.5, 10.0, 2.0
    ck = _Clock()
    pts = synth.nodes_time(N)
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(M)
    moving = [j for j in range(M) if kinds[j] in (6, 7)]
    appear = moving[:CYCLES]
    act = np.array(active, dtype=np.uint8).copy()
    act[appear] = 0                                  # the moving obstacles the robot has not seen yet
    act[hidden] = 1                                  # static ones are all known (as bench.py sets them)
    root = int(np.argmin(pts[:, 2]))
    with ck("oracle_trees"):
        trees = oracle.TreeSet(4, pts, wraps=[3], wrap_points=[2.0 * math.pi])
    with Context(4, node_capacity=N + 3 * B) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(synth.V_MIN, synth.V_MAX)
        ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
        ctx.nodes_append(pts)
        with ck("mirror"):
            es, ee = _mirror(ctx, oracle, trees, 0, pts, r_graph)
        E0 = len(es)
        assert E0 > SCAN_BLOCKS and E0 > 5 * DUB_CHUNK
        with ck("oracle_costs"):
            dist0, w_orig = _dubins_time_costs(oracle, pts, es, ee, r_min)
        w = w_orig.copy()
        assert ctx.graph_edges_append(es, ee) == 0
        assert ctx.n_graph_edges == E0
        # the steering of every mirrored edge (six chunks of 2^21) against the oracle's edge.dist
        with ck("device_steer"):
            st = ctx.dubins_steer_full(pts[es], pts[ee], r_min)
        assert st["dist"].shape == dist0.shape and np.array_equal(st["dist"], dist0), _first_diff(st["dist"], dist0)
        del st, dist0
        _report("scene", nodes=N, edges=E0, obstacles=M, seconds=ck.seconds())

        # 1. the full solve
        ck = _Clock()
        ctx.graph_edges_set_dist(0, w)
        with ck("device"):
            lmc, par, passes = ctx.graph_cost_to_root(root)
        with ck("oracle"):
            G = _solve(oracle, N, es, ee, w, root)
        cnt = _compare(lmc, par, G, es, ee, w, root, "full solve")
        assert cnt["reachable"] >= N // 2
        _report("full_solve", passes=passes, **cnt, seconds=ck.seconds())

        # 2. cycles: an obstacle appears, sweep (two-call path), block, update against the reference's own sequence
        max_cand = 0
        for i, j in enumerate(appear):
            ck = _Clock()
            act[j] = 1
            ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
            ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=act)
            with ck("oracle_sweep"):
                mask = _mask(N, oracle.points_in_conflict_polygon(trees.trees[0], ps, j, rr, delta, True, True))
                cand = int(mask[es].sum())
                want = oracle.sweep_edges_batch(pts, es, ee, mask, ps, j, rr, edge=oracle.EDGE_DUBINS_TIME, r_min=r_min)
            with ck("device_sweep"):
                ids = ctx.obstacle_sweep_polygon(j, rr, delta, r_min=r_min, cap=1 << 16)
            dev_cand = int(ctx.stats().last_sweep_candidates)
            assert np.array_equal(ids, want), (i, j, len(ids), len(want))
            max_cand = max(max_cand, cand)
            with ck("device_block_update"):
                ctx.graph_edges_block(ids)
                lmc_new, par, passes = ctx.graph_cost_update(root)
            w[want] = INF
            with ck("oracle_reference"):
                _reference_block(G, N, root, want)
            cnt = _compare(lmc_new, par, G, es, ee, w, root, f"cycle {i}")
            if i == 0:
                with ck("oracle_fresh"):
                    F = _solve(oracle, N, es, ee, w, root)
                _compare(lmc_new, par, F, es, ee, w, root, "cycle 0, fresh solve")
                del F
            _report("cycle", cycle=i, obstacle=j, candidates=cand, device_candidates=dev_cand, blocked=len(ids),
                    passes=passes, lmc_changed=int((lmc_new != lmc).sum()), **cnt, seconds=ck.seconds())
            lmc = lmc_new
        assert max_cand > DUB_CHUNK
        del G

        # 3. growth: batches of samples join the tree with both edges to every node within r_graph
        s_all, e_all, w_orig_all, p_all = es, ee, w_orig, pts
        appended = 0
        thr = TAIL_BASE + E0 // 8
        for g_i, n_batches in enumerate((1, 2)):
            ck = _Clock()
            for b in range(n_batches):
                with ck("oracle_edges"):
                    q = synth.nodes_time(B, seed=synth.SEED + 101 + 17 * (g_i * 2 + b))
                    first_node = len(p_all)
                    p_all = np.concatenate([p_all, q])
                    trees.insert_many(q)
                assert ctx.nodes_append(q) == first_node
                with ck("mirror"):
                    s_new, e_new = _mirror(ctx, oracle, trees, first_node, q, r_graph)
                with ck("oracle_edges"):
                    _, w_new = _dubins_time_costs(oracle, p_all, s_new, e_new, r_min)
                with ck("device_append"):
                    assert ctx.graph_edges_append(s_new, e_new) == len(s_all)
                    ctx.graph_edges_set_dist(len(s_all), w_new)
                s_all = np.concatenate([s_all, s_new])
                e_all = np.concatenate([e_all, e_new])
                w_orig_all = np.concatenate([w_orig_all, w_new])
                w = np.concatenate([w, w_new])
                appended += len(s_new)
            # the first growth stays below the in-edge CSR rebuild threshold (tail pass), the second goes past it
            assert (appended < thr) if g_i == 0 else (appended > thr), (appended, thr)
            with ck("device_update"):
                lmc_new, par, passes = ctx.graph_cost_update(root)
            with ck("oracle_fresh"):
                F = _solve(oracle, len(p_all), s_all, e_all, w, root)
            cnt = _compare(lmc_new, par, F, s_all, e_all, w, root, f"growth {g_i}")
            del F
            _report("growth", growth=g_i, batches=n_batches, appended_since_full_solve=appended, threshold=thr,
                    passes=passes, lmc_changed=int((lmc_new[:len(lmc)] != lmc).sum() + len(lmc_new) - len(lmc)),
                    **cnt, seconds=ck.seconds())
            lmc = lmc_new
        n_all = len(p_all)

        # 4. two of the obstacles that appeared are removed: sweep while still in use, restore, deactivate, update
        for j in appear[:2]:
            ck = _Clock()
            ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=act)
            with ck("oracle_sweep"):
                mask = _mask(n_all, oracle.points_in_conflict_polygon(trees.trees[0], ps, j, rr, delta, True, True))
                cand = int(mask[s_all].sum())
                want = oracle.sweep_edges_batch(p_all, s_all, e_all, mask, ps, j, rr, edge=oracle.EDGE_DUBINS_TIME,
                                                remove=True, dist=w, r_min=r_min)
            with ck("device_sweep"):
                freed = ctx.obstacle_sweep_polygon(j, rr, delta, r_min=r_min, remove=True, cap=1 << 16)
            assert np.array_equal(freed, want), (j, len(freed), len(want))
            assert len(freed) > 0
            w[freed] = w_orig_all[freed]
            with ck("device_update"):
                for run in _runs(freed):
                    ctx.graph_edges_set_dist(int(run[0]), w[run])
                act[j] = 0
                ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
                lmc_new, par, passes = ctx.graph_cost_update(root)
            with ck("oracle_fresh"):
                F = _solve(oracle, n_all, s_all, e_all, w, root)
            cnt = _compare(lmc_new, par, F, s_all, e_all, w, root, f"removal {j}")
            del F
            _report("removal", obstacle=j, candidates=cand, freed=len(freed), passes=passes,
                    lmc_changed=int((lmc_new != lmc).sum()), **cnt, seconds=ck.seconds())
            lmc = lmc_new
    _report("c5_total", seconds=round(time.perf_counter() - t_start, 1))


def test_c4_sphere_sweeps_block_and_update(oracle):
    """C4's tree (200 k nodes in 3-D, the mirror of every pair within the ball radius, SimpleEdge costs): the full
    solve, every one of 256 sphere sweeps against the batch sweep, the root rule at the search range, the union of the
    swept edges blocked, and the update against the reference's own sequence."""
    t_start = time.perf_counter()
    N = 200_000
    ck = _Clock()
    pts = synth.nodes(N, 3)
    r = synth.ball_radius(N, 3)
    sph = synth.spheres(256)
    # two more: the root lies exactly at sphere 256's search range, one ulp beyond sphere 257's
    extra = np.array([[pts[0, 0] + 2.0, pts[0, 1], pts[0, 2], 1.5]] * 2)
    sph = np.concatenate([sph, extra])
    d0 = float(np.sqrt(((sph[256, :3] - pts[0]) ** 2).sum()))
    ranges = np.r_[RR + DELTA + sph[:256, 3], d0, np.nextafter(d0, 0)]
    obs = oracle.make_spheres(sph)
    trees = oracle.TreeSet(3, pts)
    root, cap = 0, 1024
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph, np.ones(len(sph), dtype=np.uint8))
        with ck("mirror"):
            es, ee = _mirror(ctx, oracle, trees, 0, pts, r)
        E0 = len(es)
        assert E0 > 4 * SCAN_BLOCKS
        w = _edge_dist(pts, es, ee)                      # the SimpleEdge cost graph_edges_append gives every edge
        assert ctx.graph_edges_append(es, ee) == 0
        with ck("device_solve"):
            lmc0, par, passes = ctx.graph_cost_to_root(root)
        with ck("oracle_solve"):
            G = _solve(oracle, N, es, ee, w, root)
        cnt = _compare(lmc0, par, G, es, ee, w, root, "C4 full solve")
        _report("c4_full_solve", passes=passes, **cnt, seconds=ck.seconds())

        ck = _Clock()
        swept, cands, two_call = [], 0, 0
        for j in range(len(sph)):
            with ck("oracle_sweeps"):
                idx, _ = trees.trees[0].within_range(ranges[j], sph[j, :3])
                mask = _mask(N, idx)
                want = oracle.sweep_edges_batch(pts, es, ee, mask, obs, j, RR)
            with ck("device_sweeps"):
                got = ctx.obstacle_sweep(j, ranges[j], RR, cap=cap)
            assert np.array_equal(got, want), (j, len(got), len(want))
            if j == 256:
                assert mask[root] and (es[want] == root).any()
            if j == 257:
                assert not mask[root] and not (es[want] == root).any()
            cands += int(mask[es].sum())
            two_call += len(want) > cap
            swept.append(want)
        assert two_call >= 1
        blocked = np.unique(np.concatenate(swept))
        w[blocked] = INF
        with ck("device_block_update"):
            ctx.graph_edges_block(blocked)
            lmc, par, passes = ctx.graph_cost_update(root)
        with ck("oracle_reference"):
            _reference_block(G, N, root, blocked)
        cnt = _compare(lmc, par, G, es, ee, w, root, "C4 update")
        assert np.all(lmc >= lmc0)
        _report("c4_sweeps_update", sweeps=len(sph), candidates=cands, sweeps_two_call=int(two_call),
                blocked=len(blocked), passes=passes, lmc_changed=int((lmc != lmc0).sum()), **cnt,
                seconds=ck.seconds(), total=round(time.perf_counter() - t_start, 1))


def test_lattice_beyond_two_million_nodes(oracle):
    """A jittered 3-D lattice of 130 x 130 x 125 = 2 112 500 nodes (more than 2^21, not a multiple of 2048), both
    directed edges to the six lattice neighbours, SimpleEdge costs, root at a corner: the full solve, then the parent
    edges of 300 nodes and 300 other edges blocked and the update -- pointer jumping over a forest hundreds of hops
    deep -- against the reference's own sequence."""
    t_start = time.perf_counter()
    NX, NY, NZ = 130, 130, 125
    n = NX * NY * NZ
    assert n > SCAN_TILES and n % 2048 != 0
    rng = np.random.default_rng(2112500)
    ix, iy, iz = np.meshgrid(np.arange(NX), np.arange(NY), np.arange(NZ), indexing="ij")
    grid = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1)
    pts = grid.astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3))
    node = np.arange(n, dtype=np.int64)
    nbr = []
    for axis, step in ((0, -NY * NZ), (1, -NZ), (2, -1), (2, 1), (1, NZ), (0, NY * NZ)):    # ascending end node
        lim = (NX, NY, NZ)[axis] - 1
        ok = grid[:, axis] > 0 if step < 0 else grid[:, axis] < lim
        nbr.append(np.where(ok, node + step, -1))
    nbr = np.stack(nbr, 1).ravel()
    own = np.repeat(node, 6)
    keep = nbr >= 0
    es, ee = own[keep].astype(np.int32), nbr[keep].astype(np.int32)
    w = _edge_dist(pts, es, ee)
    root = 0
    ck = _Clock()
    with Context(3, node_capacity=n) as ctx:
        ctx.nodes_append(pts)
        assert ctx.graph_edges_append(es, ee) == 0 and ctx.n_graph_edges == len(es)
        with ck("device_solve"):
            lmc0, par0, passes0 = ctx.graph_cost_to_root(root)
        with ck("oracle_solve"):
            G = _solve(oracle, n, es, ee, w, root)
        cnt = _compare(lmc0, par0, G, es, ee, w, root, "lattice full solve")
        assert cnt["reachable"] == n
        hops = np.zeros(n, dtype=np.int64)              # depth of every node in the tree of parent edges
        for v in np.argsort(lmc0, kind="stable")[1:]:
            hops[v] = hops[ee[par0[v]]] + 1
        _report("lattice_full_solve", passes=passes0, max_depth=int(hops.max()), **cnt, seconds=ck.seconds())
        assert hops.max() > 300

        ck = _Clock()
        victims = rng.choice(np.flatnonzero(par0 >= 0), 300, replace=False)
        blocked = np.unique(np.concatenate([par0[victims], rng.choice(len(es), 300, replace=False)]))
        w[blocked] = INF
        with ck("device_block_update"):
            ctx.graph_edges_block(blocked)
            lmc, par, passes = ctx.graph_cost_update(root)
        with ck("oracle_reference"):
            _reference_block(G, n, root, blocked)
        cnt = _compare(lmc, par, G, es, ee, w, root, "lattice update")
        changed = int((lmc != lmc0).sum())
        assert np.all(lmc >= lmc0) and changed > 300
        _report("lattice_update", blocked=len(blocked), passes=passes, lmc_changed=changed, **cnt, seconds=ck.seconds(),
                total=round(time.perf_counter() - t_start, 1))
