"""Soak of the obstacle sweeps and releases on a lattice: the six entry points that walk the edge mirror
(rrtx_obstacle_sweep, _sweep_batch, _release_batch, _sweep_polygon, _sweep_polygon_batch, _release_polygon_batch) on scenes whose every
coordinate is a multiple of 1/4 (polygon centres: of 1/8) and whose ranges are distances between lattice points.  Random
real scenes never put a node exactly at an obstacle's search range, an edge exactly tangent to an inflated sphere or an
edge along a polygon's side; here many are, so the strict / non-strict decisions of the mark kernels, the per-bit root
rule of the 64-obstacle words and the edge tests fed from the mirror all decide rows.

Three scenes, each built WITH its oracle answers by a function that needs no device (sphere_scene, polygon_scene,
dubins_scene; *_conditions count, on the oracle and in exact integer arithmetic alone, the boundary cases a scene
holds), and each compared through the C-ABI by another (check_spheres, check_polygons, check_dubins), bit for bit.
The moving kinds 6 / 7 (RRTX_OPT_SPACE_HAS_TIME) are not covered here."""
import math
import os
import sys
import time
import types
from fractions import Fraction

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, ".."))
sys.path.insert(0, _HERE)
from oracle import oracle as O  # noqa: E402
from soak_lattice import lattice, lattice_polygons  # noqa: E402

BUMP = 2.0 ** -30                      # one ulp of DELTA rounds away in (RR + DELTA) + radius; this does not
RANGES = (1.25, 2.5, 3.25, 3.75)       # lattice hypotenuses (3-4-5, 5-12-13, 9-12-15 in quarters)
BOX_SIDES = ((0.75, 1.0), (1.5, 2.0), (3.0, 4.0), (2.0, 1.5), (1.25, 3.0))     # half diagonals 0.625 / 1.25 / 2.5 / 1.25 / 1.625
ROOT_OB = 3                            # the list position whose range the root lies on exactly


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _i8(a):
    """coordinates x 8 as integers (exact: everything here is a multiple of 1/8)"""
    a8 = np.asarray(a, dtype=np.float64) * 8.0
    r = np.rint(a8)
    assert np.array_equal(a8, r), "a coordinate that is no multiple of 1/8"
    return r.astype(np.int64)


def thr_first_ge(r):
    """the smallest double s with sqrt(s) >= r: a node is within r exactly when its squared distance is below it"""
    s = float(r) * float(r)
    while math.sqrt(np.nextafter(s, 0.0)) >= r:
        s = float(np.nextafter(s, 0.0))
    while math.sqrt(s) < r:
        s = float(np.nextafter(s, np.inf))
    return s


def le_sensitive(r):
    """a node exactly at range r has squared distance r * r; `s <= thr` in place of `s < thr` takes it only where the
    threshold IS r * r, i.e. where sqrt of the double below r * r already rounds below r (mantissa of r above sqrt 2:
    3.25 and 3.75 of RANGES; 1.25 and 2.5 have their threshold one ulp below r * r)"""
    return thr_first_ge(r) == float(r) * float(r)


def _graph(rng, tree, pts, reach, per_node, toward):
    """per_node out-edges of every node to nodes the oracle finds within `reach`; the root's go to the neighbours
    nearest to `toward` (the obstacle it lies on the range of); edge per_node is a zero-length one"""
    n = len(pts)
    es = np.repeat(np.arange(n), per_node).astype(np.int32)
    ee = es.copy()
    for i in range(n):
        idx = np.sort(tree.within_range(reach, pts[i])[0])
        idx = idx[idx != i]
        if len(idx) == 0:
            continue
        if i == 0:
            d = ((pts[idx] - toward) ** 2).sum(axis=1)
            pick = idx[np.argsort(d, kind="stable")][:per_node]
            pick = np.resize(pick, per_node)
        else:
            pick = rng.choice(idx, per_node, replace=len(idx) < per_node)
        ee[i * per_node:(i + 1) * per_node] = pick
    ee[per_node] = es[per_node]
    return es, ee


def _order(rng, K, at_63, in_second, at_62=None):
    """all K positions shuffled, with `at_63` at index 63 (the last bit of the first 64-obstacle word), `in_second` at
    index 64 (the second word) and `at_62` at index 62"""
    order = rng.permutation(K).astype(np.int32)
    for pos, where in ((at_63, 63), (in_second, 64), (at_62, 62)):
        if pos is None or where >= K:
            continue
        a = int(np.flatnonzero(order == pos)[0])
        order[a], order[where] = order[where], order[a]
    return order


# ---- scene S: spheres, dim = 3 ----------------------------------------------------------------------------------------
def _mask(tree, n, r, c):
    m = np.zeros(n, dtype=np.uint8)
    m[tree.within_range(float(r), c)[0]] = 1
    return m


def tangent_matrix(pts8, es, ee, sph, rr):
    """[K, ne] bool, in integers: the exact squared distance of mirrored edge e to the centre of sphere j equals
    (radius + rr)^2: |p - c|^2 L^2 - ((c - p) . d)^2 == R^2 L^2 inside the segment, the endpoint distance outside"""
    P, E = pts8[es], pts8[ee]
    d = E - P
    L2 = (d * d).sum(axis=1)
    out = np.zeros((len(sph), len(es)), dtype=bool)
    for j in range(len(sph)):
        c = _i8(sph[j, :3])
        R2 = int(_i8(sph[j, 3] + rr)) ** 2
        w = c - P
        ww = (w * w).sum(axis=1)
        dot = (w * d).sum(axis=1)
        we = ((c - E) ** 2).sum(axis=1)
        inside = (dot > 0) & (dot < L2)
        out[j] = np.where(inside, ww * L2 - dot * dot == R2 * L2, np.where(dot <= 0, ww == R2, we == R2))
    return out


def sphere_scene(seed, n_draw=3000, span=6, K=70, rr=0.5, n_blocked=40):
    """Scene S with its oracle rows.  Node 0 is the root and lies exactly at search[ROOT_OB] from sphere ROOT_OB."""
    rng = np.random.default_rng(seed)
    s = types.SimpleNamespace(seed=seed, K=K, rr=rr)
    pts = np.unique(lattice(rng, span, (n_draw, 3)), axis=0)
    s.pts = pts = pts[rng.permutation(len(pts))]
    s.n = n = len(pts)
    s.tree = O.KDTree(3)
    s.tree.insert_many(pts)
    sph = np.c_[lattice(rng, span - 1, (K, 3)), rng.integers(1, 9, K) / 4.0]
    search = rng.choice(RANGES, K)
    sph[ROOT_OB] = [*(pts[0] + [0.75, 1.0, 0.0]), 2.0]
    search[ROOT_OB] = 1.25
    s.sph, s.search = sph, search
    s.active = np.ones(K, dtype=np.uint8)
    s.active[min(11, K - 1) if min(11, K - 1) != ROOT_OB else 0] = 0
    s.es, s.ee = _graph(rng, s.tree, pts, 2.0, 7, sph[ROOT_OB, :3])
    s.osph = O.make_spheres(sph, s.active)
    s.search_up = np.nextafter(search, np.inf)
    s.search_dn = np.nextafter(search, 0.0)
    s.rows, s.rows_up, s.rows_dn = (
        [O.sweep_edges_batch(pts, s.es, s.ee, _mask(s.tree, n, r[j], sph[j, :3]), s.osph, j, rr) for j in range(K)]
        for r in (search, s.search_up, s.search_dn))
    changed = [j for j in range(K) if not np.array_equal(s.rows[j], s.rows_up[j]) and j != ROOT_OB]
    s.changed = changed
    s.changed_le = hot = [j for j in changed if le_sensitive(search[j])]         # the rows a `<=` for every node changes
    s.order = _order(rng, K, hot[0] if hot else None, hot[1] if len(hot) > 1 else None, ROOT_OB)
    # ---- the release: blocked = what the sweeps of positions 0 .. n_blocked - 1 return; 66 entries leave (64 + 2):
    # the even positions below n_blocked, position 63 and one position of the second word, repeats to fill ----
    nb = min(n_blocked, K)
    s.blocked = np.unique(np.concatenate([s.rows[j] for j in range(nb)] + [np.zeros(0, np.int32)])).astype(np.int32)
    s.dist_host = np.ones(len(s.es))
    s.dist_host[s.blocked] = np.inf
    distinct = [j for j in range(0, nb, 2) if j != ROOT_OB] + [j for j in (63, 66) if j < K]
    L = np.array(distinct, dtype=np.int32)
    if K > 64:
        L = np.resize(L, 66)
        hot = [j for j in distinct if len(_release_row(s, distinct, j)) > 0]   # entries 63 and 64 free something
        if hot:
            L[63], L[64] = hot[0], hot[-1]
    s.leaving = L
    s.lsearch = search[L]
    s.release = [_release_row(s, L, int(p)) for p in L]
    return s


def _release_row(s, leaving, pos):
    a = s.active.copy()
    a[np.asarray(leaving, dtype=np.int64)] = 0
    a[pos] = 1
    return O.sweep_edges_batch(s.pts, s.es, s.ee, _mask(s.tree, s.n, s.search[pos], s.sph[pos, :3]),
                               O.make_spheres(s.sph, a), int(pos), s.rr, remove=True, dist=s.dist_host)


def sphere_conditions(s):
    """what scene S holds on the thresholds, from the oracle's rows and integers alone"""
    pts8 = _i8(s.pts)
    K, ne = s.K, len(s.es)
    d2 = ((pts8[None, :, :] - _i8(s.sph[:, :3])[:, None, :]) ** 2).sum(axis=2)          # [K, n]
    on = d2 == (_i8(s.search) ** 2)[:, None]
    tang = tangent_matrix(pts8, s.es, s.ee, s.sph, s.rr)
    in_range = np.stack([_mask(s.tree, s.n, s.search[j], s.sph[j, :3]) for j in range(K)]).astype(bool)
    tang_in = tang & in_range[:, s.es] & (s.active[:, None] != 0)
    idx_of = {int(p): i for i, p in enumerate(s.order)}
    root_out = np.flatnonzero(s.es == 0)
    out = {
        "nodes": s.n, "edges": ne, "ids": int(sum(len(r) for r in s.rows)),
        "on_range": int(on[:, 1:].sum()), "root_on_range": bool(on[ROOT_OB, 0]),
        "rows_changed_up": len(s.changed), "changed_batch_index": sorted(idx_of[j] for j in s.changed),
        "rows_changed_le": len(s.changed_le), "changed_le_batch_index": sorted(idx_of[j] for j in s.changed_le),
        "tangent_edges": int(tang_in.any(axis=0).sum()), "tangent_rows": int(tang_in.any(axis=1).sum()),
        "root_row": np.intersect1d(s.rows[ROOT_OB], root_out), "root_row_dn": np.intersect1d(s.rows_dn[ROOT_OB], root_out),
    }
    # the release
    L = np.unique(s.leaving)
    stay = s.active.copy()
    stay[L] = 0
    one = np.zeros(K, dtype=np.uint8)
    hits13 = []
    for p in L:                                     # conditions 1-3 of the header: blocked, in range of p, hitting p
        a = one.copy()
        a[p] = 1
        h = O.sweep_edges_batch(s.pts, s.es, s.ee, in_range[p].astype(np.uint8), O.make_spheres(s.sph, a), int(p), s.rr)
        hits13.append(np.intersect1d(h, s.blocked))
    hits13 = np.unique(np.concatenate(hits13))
    freed = np.unique(np.concatenate(s.release))
    out.update(release_candidates=len(hits13), release_freed=len(freed), release_held=len(np.setdiff1d(hits13, freed)),
               release_tangent_to_staying=int(tang[stay != 0][:, hits13].any(axis=0).sum()),
               release_row_63=len(s.release[63]) if len(s.release) > 64 else -1,
               release_rows_second=int(sum(len(r) for r in s.release[64:])),
               leaving_has_63=bool(63 in L), leaving_second=[int(p) for p in L if p >= 64])
    return out


def check_spheres(s, solve=True):
    """scene S through the C-ABI against its oracle rows; returns counts"""
    from rrtqx_3d_amd.context import Context
    out = {"rows": 0, "ids": 0}
    order = s.order
    with Context(3) as ctx:
        ctx.nodes_append(s.pts)
        ctx.spheres_set(s.sph, s.active)
        assert ctx.graph_edges_append(s.es, s.ee) == 0
        total = sum(len(s.rows[p]) for p in order)
        for cap in (16, total):                                      # the two-call path; exactly enough
            rows = _rows_of(*ctx.obstacle_sweep_batch(order, s.search[order], s.rr, cap=cap))
            for j, p in enumerate(order):
                assert np.array_equal(rows[j], s.rows[p]), f"scene {s.seed}: sweep row {j} (sphere {p}) differs"
        for j, p in enumerate(order):
            assert np.array_equal(ctx.obstacle_sweep(int(p), float(s.search[p]), s.rr), rows[j]), \
                f"scene {s.seed}: single sweep of sphere {p} differs"
        out["rows"] += len(order); out["ids"] += total
        for name, search, want in (("up", s.search_up, s.rows_up), ("down", s.search_dn, s.rows_dn)):
            rows = _rows_of(*ctx.obstacle_sweep_batch(order, search[order], s.rr))
            for j, p in enumerate(order):
                assert np.array_equal(rows[j], want[p]), f"scene {s.seed}: sweep row {j} (sphere {p}), range one ulp {name}, differs"
                if p in s.changed or p == ROOT_OB:
                    assert np.array_equal(ctx.obstacle_sweep(int(p), float(search[p]), s.rr), want[p]), \
                        f"scene {s.seed}: single sweep of sphere {p}, range one ulp {name}, differs"
            out["rows"] += len(order); out["ids"] += sum(len(r) for r in rows)
        # one sphere alone over the mirror's index pairs
        for p in [p for p in order if s.active[p]][:10]:
            a = np.zeros(s.K, dtype=np.uint8)
            a[p] = 1
            hit, _ = ctx.edges_check_idx(s.es, s.ee, s.rr, obstacle=int(p))
            want, _ = O.edges_check_spheres(*O.make_spheres(s.sph, a), s.pts[s.es], s.pts[s.ee], s.rr)
            assert np.array_equal(hit, want), f"scene {s.seed}: edges_check_idx against sphere {p} differs"
        # the release of the leaving set
        nb = min(40, s.K)
        off, ids = ctx.obstacle_sweep_batch(np.arange(nb, dtype=np.int32), s.search[:nb], s.rr, block=True)
        assert np.array_equal(np.unique(ids), s.blocked)
        rtotal = sum(len(r) for r in s.release)
        for cap in (16, max(rtotal, 1)):
            rows = _rows_of(*ctx.obstacle_release_batch(s.leaving, s.lsearch, s.rr, cap=cap))
            for j, p in enumerate(s.leaving):
                assert np.array_equal(rows[j], s.release[j]), f"scene {s.seed}: release row {j} (sphere {p}) differs"
        out["rows"] += len(s.leaving); out["ids"] += rtotal
    if solve:
        check_spheres_marks(s)
    return out


def _solved(oracle_lmc, oracle_par, lmc, par, es, ee, w, root, what):
    assert np.array_equal(lmc, oracle_lmc), f"{what}: rrtLMC differs from the oracle's solve"
    ok = np.isfinite(w) & np.isfinite(lmc[ee]) & np.isfinite(lmc[es]) & (es != root)
    att = np.flatnonzero(ok & (np.where(ok, lmc[ee] + np.where(ok, w, 0.0), np.inf) == lmc[es]))
    single = np.bincount(es[att], minlength=len(lmc)) == 1           # where one edge alone attains the minimum
    assert np.array_equal(par[single], oracle_par[single]), f"{what}: parent edges differ"


def check_spheres_marks(s):
    """block=True of the sweeps of positions 0 .. 39 against rrtx_graph_edges_block(union) on a second context, then
    unblock=True of the scene's leaving set against rrtx_graph_edges_unblock(union), through the cost solve that reads
    the marks (root 0): equal rrtLMC from both contexts, equal to the oracle's solve, parent edges where a single edge
    attains the minimum."""
    from rrtqx_3d_amd.context import Context
    es, ee = s.es, s.ee

    def solve(w):
        g = O.Graph(s.n + 1)                             # node n: a goal that stays at Inf, so the queue runs dry
        g.add_edges(es, ee, w)
        for v in range(s.n + 1):
            g.set_node(v, np.inf, np.inf)
        g.set_node(0, 0.0, np.inf)
        g.verifyInQueue(0)
        g.reduceInconsistency(s.n, 0)
        return g.lmc()[:s.n], g.parent_edge()[:s.n]

    d = s.pts[es] - s.pts[ee]
    w0 = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    nb = min(40, s.K)
    sweep = np.arange(nb, dtype=np.int32)
    w_b = w0.copy()
    w_b[s.blocked] = np.inf
    funion = np.unique(np.concatenate(s.release)).astype(np.int32)
    w_u = w_b.copy()
    w_u[funion] = w0[funion]
    want_b, want_u = solve(w_b), solve(w_u)
    ctxs = []
    try:
        for _ in range(2):
            c = Context(3)
            ctxs.append(c)
            c.nodes_append(s.pts)
            c.spheres_set(s.sph, s.active)
            assert c.graph_edges_append(es, ee) == 0
            c.graph_cost_to_root(0)
        c1, c2 = ctxs
        got = _rows_of(*c1.obstacle_sweep_batch(sweep, s.search[:nb], s.rr, block=True))
        for j in range(nb):
            assert np.array_equal(got[j], s.rows[j]), f"scene {s.seed}: sweep row {j} with block=True differs"
        c2.graph_edges_block(s.blocked)
        for c, what in ((c1, "block=True"), (c2, "graph_edges_block(union)")):
            lmc, par, _ = c.graph_cost_update(0)
            _solved(*want_b, lmc, par, es, ee, w_b, 0, f"scene {s.seed}, {what}")
        got = _rows_of(*c1.obstacle_release_batch(s.leaving, s.lsearch, s.rr, unblock=True))
        for j in range(len(s.leaving)):
            assert np.array_equal(got[j], s.release[j]), f"scene {s.seed}: release row {j} with unblock=True differs"
        c2.graph_edges_unblock(funion)
        for c, what in ((c1, "unblock=True"), (c2, "graph_edges_unblock(union)")):
            lmc, par, _ = c.graph_cost_update(0)
            _solved(*want_u, lmc, par, es, ee, w_u, 0, f"scene {s.seed}, {what}")
        assert len(c1.obstacle_release_batch(s.leaving, s.lsearch, s.rr)[1]) == 0    # what was freed is no longer blocked
    finally:
        for c in ctxs:
            c.close()
    return {"blocked": len(s.blocked), "freed": len(funion), "lmc_changed_by_block": int((want_b[0] != solve(w0)[0]).sum()),
            "lmc_changed_by_unblock": int((want_u[0] != want_b[0]).sum())}


# ---- scene P: the polygon list, SimpleEdge, dim = 3 at z = 0 --------------------------------------------------------------
def _box(corner, w, h):
    x, y = corner
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float64)


def polygon_scene(seed, n_draw=2500, span=8, K=70, rr=0.5, delta=0.75, n_other=14):
    """Scene P with its oracle rows.  Node 0 is the root and lies exactly on the range of box ROOT_OB."""
    rng = np.random.default_rng(seed)
    s = types.SimpleNamespace(seed=seed, K=K, rr=rr, delta=delta, delta_up=delta + BUMP, delta_dn=delta - BUMP)
    xy = np.unique(lattice(rng, span, (n_draw, 2)), axis=0)
    xy = xy[rng.permutation(len(xy))]
    s.pts = pts = np.c_[xy, np.zeros(len(xy))]
    s.n = len(pts)
    s.tree = O.KDTree(3)
    s.tree.insert_many(pts)
    polys, kinds, sides = [], [], []
    for j in range(K):
        w, h = BOX_SIDES[int(rng.integers(0, len(BOX_SIDES)))]
        polys.append(_box(lattice(rng, span - 2, 2), w, h))
        kinds.append(3); sides.append((w, h))
    # the root's box: sides (1.5, 2), centre on the lattice, range (rr + delta) + 1.25; the root at (2, 1.5) from its
    # centre is a 3-4-5 triple in halves, exactly 2.5 away when rr + delta = 1.25
    polys[ROOT_OB] = _box(xy[0] - [2.0, 1.5] - [0.75, 1.0], 1.5, 2.0)
    sides[ROOT_OB] = (1.5, 2.0)
    other, okinds = lattice_polygons(rng, n_other, span - 2)          # right triangles, diamonds, boxes; some kind-1 balls
    where = [j for j in rng.permutation(K) if j not in (ROOT_OB, 63)][:n_other]
    s.is_box = np.ones(K, dtype=bool)
    for j, p, k in zip(where, other, okinds):
        polys[j], kinds[j] = p, k
        s.is_box[j] = False
    s.polys, s.kinds, s.sides = polys, kinds, sides
    s.active = np.ones(K, dtype=np.uint8)
    s.active[[j for j in (17, 41) if j < K and j != ROOT_OB]] = 0
    s.ps = O.PolygonSet(polys, kinds=kinds, active=s.active)
    s.cr = s.ps.centre_radius()
    s.es, s.ee = _graph(rng, s.tree, pts, 3.0, 6, np.r_[s.cr[ROOT_OB, :2], 0.0])
    s.rows, s.rows_up = ([O.add_new_obstacle_edges(s.tree, pts, s.es, s.ee, s.ps, j, rr, d, dubins=False) for j in range(K)]
                         for d in (delta, s.delta_up))
    s.root_row_dn = O.add_new_obstacle_edges(s.tree, pts, s.es, s.ee, s.ps, ROOT_OB, rr, s.delta_dn, dubins=False)
    s.changed = [j for j in range(K) if not np.array_equal(s.rows[j], s.rows_up[j]) and j != ROOT_OB]
    s.changed_le = hot = [j for j in s.changed if s.is_box[j] and le_sensitive((rr + delta) + s.cr[j, 2])]
    s.order = _order(rng, K, hot[0] if hot else None, hot[1] if len(hot) > 1 else None, ROOT_OB)
    # mode 1 after the union of the first 20 rows is blocked
    nb = min(20, K)
    s.blocked = np.unique(np.concatenate(s.rows[:nb] + [np.zeros(0, np.int32)])).astype(np.int32)
    s.blocked_up = np.unique(np.concatenate(s.rows_up[:nb] + [np.zeros(0, np.int32)])).astype(np.int32)
    s.removed = list(range(0, nb, 2))
    s.remove_rows, s.remove_rows_up = [], []
    for d, blocked, dst in ((delta, s.blocked, s.remove_rows), (s.delta_up, s.blocked_up, s.remove_rows_up)):
        dist = np.ones(len(s.es))
        dist[blocked] = np.inf
        for j in s.removed:
            dst.append(O.remove_obstacle_edges(s.tree, pts, s.es, s.ee, dist, s.ps, j, rr, d, dubins=False))
    return s


def _seg_dist2(p, q, a, b):
    """exact squared distance between segments pq and ab (integer points), as a Fraction"""
    def pt_seg(x, a, b):
        ux, uy = b[0] - a[0], b[1] - a[1]
        vx, vy = x[0] - a[0], x[1] - a[1]
        L2, dot = ux * ux + uy * uy, vx * ux + vy * uy
        if L2 == 0 or dot <= 0:
            return Fraction(vx * vx + vy * vy)
        if dot >= L2:
            return Fraction((x[0] - b[0]) ** 2 + (x[1] - b[1]) ** 2)
        return Fraction((vx * vx + vy * vy) * L2 - dot * dot, L2)

    def orient(a, b, c):
        v = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        return (v > 0) - (v < 0)
    o1, o2, o3, o4 = orient(p, q, a), orient(p, q, b), orient(a, b, p), orient(a, b, q)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return Fraction(0)
    return min(pt_seg(p, a, b), pt_seg(q, a, b), pt_seg(a, p, q), pt_seg(b, p, q))


def polygon_conditions(s):
    """what scene P holds on the thresholds, from the oracle's rows and integers alone (boxes only: their centres are
    on the 1/8 grid and their radii exact)"""
    pts8 = _i8(s.pts[:, :2])
    box = np.flatnonzero(s.is_box)
    half = np.array([math.hypot(w / 2.0, h / 2.0) for w, h in s.sides])
    assert np.array_equal(s.cr[box, 2], half[box]) and set(half[box]) <= {0.625, 1.25, 1.625, 2.5}
    rng8 = _i8((s.rr + s.delta) + s.cr[box, 2])
    d2 = ((pts8[None, :, :] - _i8(s.cr[box, :2])[:, None, :]) ** 2).sum(axis=2)
    on = d2 == (rng8 ** 2)[:, None]
    idx_of = {int(p): i for i, p in enumerate(s.order)}
    root_out = np.flatnonzero(s.es == 0)
    # edges of a box's candidates that lie along one of its sides, pass through one of its vertices, or keep exactly rr
    # from a side
    rr2 = Fraction(int(_i8(s.rr)) ** 2)
    along = through = at_rr = 0
    special = set()
    for j in [j for j in box if s.active[j]][:16]:                   # (the first 16 boxes in use hold plenty)
        nodes = O.points_in_conflict_polygon(s.tree, s.ps, int(j), s.rr, s.delta, False, False)
        v8 = _i8(s.polys[j])
        for e in np.flatnonzero(np.isin(s.es, nodes)):
            p, q = pts8[s.es[e]].tolist(), pts8[s.ee[e]].tolist()
            if p == q:
                continue
            dx, dy = q[0] - p[0], q[1] - p[1]
            cr = [dx * (v[1] - p[1]) - dy * (v[0] - p[0]) for v in v8.tolist()]
            dt = [dx * (v[0] - p[0]) + dy * (v[1] - p[1]) for v in v8.tolist()]
            L2 = dx * dx + dy * dy
            is_through = any(c == 0 and 0 <= t <= L2 for c, t in zip(cr, dt))
            is_along = any(cr[k] == 0 and cr[(k + 1) % 4] == 0 and max(dt[k], dt[(k + 1) % 4]) >= 0 and min(dt[k], dt[(k + 1) % 4]) <= L2
                           for k in range(4))
            d2s = [_seg_dist2(p, q, v8[k].tolist(), v8[(k + 1) % 4].tolist()) for k in range(4)]
            is_rr = min(d2s) == rr2 and rr2 > 0
            along += is_along; through += is_through and not is_along; at_rr += is_rr
            if is_along or is_through or is_rr:
                special.add(int(e))
    return {
        "nodes": s.n, "edges": len(s.es), "ids": int(sum(len(r) for r in s.rows)),
        "on_range": int(on[:, 1:].sum()), "root_on_range": bool(on[list(box).index(ROOT_OB), 0]),
        "rows_changed_up": len(s.changed), "changed_batch_index": sorted(idx_of[j] for j in s.changed),
        "rows_changed_le": len(s.changed_le), "changed_le_batch_index": sorted(idx_of[j] for j in s.changed_le),
        "edges_along_a_side": along, "edges_through_a_vertex": through, "edges_at_rr_from_a_side": at_rr,
        "special_edges": len(special),
        "root_row": np.intersect1d(s.rows[ROOT_OB], root_out), "root_row_dn": np.intersect1d(s.root_row_dn, root_out),
        "removed_ids": int(sum(len(r) for r in s.remove_rows)),
    }


def check_polygons(s):
    """scene P through the C-ABI against its oracle rows; returns counts"""
    from rrtqx_3d_amd.context import Context
    out = {"rows": 0, "ids": 0}
    order = s.order
    with Context(3) as ctx:
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, kinds=s.kinds, active=s.active)
        assert ctx.graph_edges_append(s.es, s.ee) == 0
        for name, d, want in (("DELTA", s.delta, s.rows), ("DELTA + 2^-30", s.delta_up, s.rows_up)):
            rows = _rows_of(*ctx.obstacle_sweep_polygon_batch(order, s.rr, d, cap=16))
            for j, p in enumerate(order):
                assert np.array_equal(rows[j], want[p]), f"scene {s.seed}: polygon row {j} (position {p}) at {name} differs"
                assert np.array_equal(ctx.obstacle_sweep_polygon(int(p), s.rr, d), rows[j]), \
                    f"scene {s.seed}: single polygon sweep of position {p} at {name} differs"
            out["rows"] += len(order); out["ids"] += sum(len(r) for r in rows)
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch([ROOT_OB, ROOT_OB], s.rr, s.delta_dn))
        assert np.array_equal(rows[0], s.root_row_dn) and np.array_equal(rows[1], s.root_row_dn), \
            f"scene {s.seed}: the root's polygon row at DELTA - 2^-30 differs"
        assert np.array_equal(ctx.obstacle_sweep_polygon(ROOT_OB, s.rr, s.delta_dn), s.root_row_dn)
        # mode 1
        for name, d, blocked, want in (("DELTA", s.delta, s.blocked, s.remove_rows),
                                       ("DELTA + 2^-30", s.delta_up, s.blocked_up, s.remove_rows_up)):
            ctx.graph_edges_unblock(np.arange(len(s.es), dtype=np.int32))
            ctx.graph_edges_block(blocked)
            for j, w in zip(s.removed, want):
                assert np.array_equal(ctx.obstacle_sweep_polygon(j, s.rr, d, remove=True, cap=8), w), \
                    f"scene {s.seed}: mode 1 of position {j} at {name} differs"
                out["rows"] += 1; out["ids"] += len(w)
    return out


# ---- scene D: Dubins, dim = 4, theta wrapped at 2 pi, static polygons ------------------------------------------------------
ORIGIN_BOXES = ((0.75, 1.0), (1.5, 2.0), (3.0, 4.0))           # centred at the origin: radii 0.625, 1.25, 2.5


def dubins_scene(seed, root_planted=False, n_draw=300, span=6, m=10, rr=0.5, delta=0.75, r_min=None):
    """Scene D with its oracle rows: lattice poses, headings multiples of pi / 4 (0 and 2 pi included), and for every
    polygon centred at the origin four planted nodes exactly on its range R = ((rr + delta) + radius) + pi:
    (+-R, 0, 0, pi) and (0, +-R, 0, pi).  root_planted: one planted node is node 0."""
    rng = np.random.default_rng(seed)
    s = types.SimpleNamespace(seed=seed, rr=rr, delta=delta, delta_up=delta + BUMP, root_planted=root_planted)
    s.r_min = float(rng.choice([0.5, 1.0, 2.0])) if r_min is None else r_min
    poses = np.zeros((n_draw, 4))
    poses[:, :2] = lattice(rng, span, (n_draw, 2))
    poses[:, 3] = rng.integers(0, 9, n_draw) * (np.pi / 4)
    poses = np.unique(poses, axis=0)
    poses = poses[rng.permutation(len(poses))]
    polys = [_box((-w / 2.0, -h / 2.0), w, h) for w, h in ORIGIN_BOXES]
    other, okinds = lattice_polygons(rng, m - len(polys), span)
    s.polys, s.kinds = polys + other, [3] * len(polys) + list(okinds)
    s.m = len(s.polys)
    s.active = np.ones(s.m, dtype=np.uint8)
    s.active[s.m - 2] = 0
    s.ps = O.PolygonSet(s.polys, kinds=s.kinds, active=s.active)
    cr = s.ps.centre_radius()
    planted, s.planted_of = [], {}
    for j in range(len(ORIGIN_BOXES)):
        assert cr[j, 0] == 0.0 and cr[j, 1] == 0.0
        R = ((rr + delta) + cr[j, 2]) + math.pi                    # as the host forms it
        s.planted_of[j] = (R, [len(planted) + k for k in range(4)])
        planted += [(R, 0.0, 0.0, math.pi), (-R, 0.0, 0.0, math.pi), (0.0, R, 0.0, math.pi), (0.0, -R, 0.0, math.pi)]
    planted = np.array(planted)
    if root_planted:                                                # planted nodes first: node 0 is one of them
        s.pts = np.concatenate([planted, poses])
        first = 0
    else:
        s.pts = np.concatenate([poses[:1], planted, poses[1:]])
        first = 1
    for j in s.planted_of:
        s.planted_of[j] = (s.planted_of[j][0], [first + k for k in s.planted_of[j][1]])
    s.planted = np.arange(first, first + len(planted))
    s.n = len(s.pts)
    s.tree = O.KDTree(4, wraps=[3], wrap_points=[2.0 * math.pi])
    s.tree.insert_many(s.pts)
    # five out-edges per node to poses within 4.0; a planted node's go to the poses nearest to the origin on the far
    # side of it, so that they cross the polygons it is on the range of
    es = np.repeat(np.arange(s.n), 5).astype(np.int32)
    ee = es.copy()
    near_origin = np.argsort((s.pts[:, :2] ** 2).sum(axis=1), kind="stable")
    near_origin = near_origin[~np.isin(near_origin, s.planted)]
    for i in range(s.n):
        if i in s.planted:
            far = near_origin[(s.pts[near_origin, :2] @ s.pts[i, :2]) <= 0.0]
            ee[5 * i:5 * i + 5] = np.resize(far[:5], 5)
            continue
        idx = np.sort(s.tree.within_range(4.0, s.pts[i])[0])
        idx = idx[idx != i]
        if len(idx):
            ee[5 * i:5 * i + 5] = rng.choice(idx, 5, replace=len(idx) < 5)
    s.es, s.ee = es, ee
    s.rows, s.rows_up = ([O.add_new_obstacle_edges(s.tree, s.pts, es, ee, s.ps, j, rr, d, dubins=True, r_min=s.r_min)
                          for j in range(s.m)] for d in (delta, s.delta_up))
    s.order = np.resize(rng.permutation(s.m), 70).astype(np.int32)         # 70 entries with repeats: a second group
    return s


def dubins_conditions(s):
    """every planted node is exactly on its polygon's range: out at DELTA (the root: in), in at DELTA + 2^-30"""
    on = 0
    rows_changed = 0
    for j, (R, nodes) in s.planted_of.items():
        assert math.sqrt(R * R) == R
        inside = set(O.points_in_conflict_polygon(s.tree, s.ps, j, s.rr, s.delta, False, True).tolist())
        inside_up = set(O.points_in_conflict_polygon(s.tree, s.ps, j, s.rr, s.delta_up, False, True).tolist())
        for i in nodes:
            p = s.pts[i]
            assert p[3] == math.pi and p[2] == 0.0 and sorted(np.abs(p[:2]).tolist()) == [0.0, R]
            assert (i in inside) == (i == 0) and i in inside_up, (j, i)
            on += 1
        rows_changed += int(not np.array_equal(s.rows[j], s.rows_up[j]))
    return {"nodes": s.n, "edges": len(s.es), "ids": int(sum(len(r) for r in s.rows)), "planted": len(s.planted),
            "planted_on_range": on, "rows_changed_up": rows_changed,
            "root_is_planted": bool(0 in s.planted)}


def check_dubins(s):
    """scene D through the C-ABI against its oracle rows; once more with RRTX_OPT_ROOT_RULE = 0, where the single calls
    are the reference (the oracle has no such mode)"""
    from rrtqx_3d_amd import _capi
    from rrtqx_3d_amd.context import Context
    out = {"rows": 0, "ids": 0}
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, kinds=s.kinds, active=s.active)
        assert ctx.graph_edges_append(s.es, s.ee) == 0
        cost, _ = ctx.dubins_steer(s.pts[s.es], s.pts[s.ee], s.r_min)
        ctx.graph_edges_set_dist(0, cost)
        for name, d, want in (("DELTA", s.delta, s.rows), ("DELTA + 2^-30", s.delta_up, s.rows_up)):
            single = [ctx.obstacle_sweep_polygon(j, s.rr, d, r_min=s.r_min) for j in range(s.m)]
            rows = _rows_of(*ctx.obstacle_sweep_polygon_batch(s.order, s.rr, d, r_min=s.r_min, cap=8))
            for j in range(s.m):
                assert np.array_equal(single[j], want[j]), f"scene {s.seed}: single Dubins sweep of position {j} at {name} differs"
            for j, p in enumerate(s.order):
                assert np.array_equal(rows[j], want[p]), f"scene {s.seed}: Dubins row {j} (position {p}) at {name} differs"
            out["rows"] += len(rows); out["ids"] += sum(len(r) for r in rows)
        ctx.set_option(_capi.RRTX_OPT_ROOT_RULE, 0)
        single = [ctx.obstacle_sweep_polygon(j, s.rr, s.delta, r_min=s.r_min) for j in range(s.m)]
        rows = _rows_of(*ctx.obstacle_sweep_polygon_batch(s.order, s.rr, s.delta, r_min=s.r_min))
        for j, p in enumerate(s.order):
            assert np.array_equal(rows[j], single[p]), f"scene {s.seed}: Dubins row {j} (position {p}) without the root rule differs"
        root_out = np.flatnonzero(s.es == 0)
        for j in range(s.m):                    # without the rule a row loses at most out-edges of node 0
            gone = np.setdiff1d(s.rows[j], single[j])
            assert np.isin(gone, root_out).all() and len(np.setdiff1d(single[j], s.rows[j])) == 0
        out["no_root_rule_lost"] = int(sum(len(np.setdiff1d(s.rows[j], single[j])) for j in range(s.m)))
    return out


# ---- the release burst (rrtx_obstacle_release_polygon_batch) on scenes P and D -------------------------------------------
def release_flags(active, entries):
    """the in-use flags the rows of a release burst are judged under: what stays = in use and not listed"""
    stay = np.array(active, dtype=np.uint8).copy()
    stay[np.asarray(entries, dtype=np.int64)] = 0
    return stay


def release_rows_reference(s, entries, dist, delta, dubins, r_min=0.0):
    """row j of the burst = remove_obstacle_edges(entries[j]) under flags where the OTHER listed positions are not in
    use (the entry itself keeps its own flag)"""
    stay = release_flags(s.active, entries)
    rows = {}
    for p in sorted(set(int(q) for q in entries)):
        flags = stay.copy()
        flags[p] = s.active[p]
        ps = O.PolygonSet(s.polys, kinds=s.kinds, active=flags)
        rows[p] = O.remove_obstacle_edges(s.tree, s.pts, s.es, s.ee, dist, ps, p, s.rr, delta, dubins=dubins, r_min=r_min)
    return [rows[int(p)] for p in entries]


def polygon_release_entries(s):
    """scene P: every second of the first 20 positions (the rows that were blocked), the positions not in use, the root's
    box and one in-use position a second time, shuffled by the scene's seed"""
    idle = [int(j) for j in np.flatnonzero(s.active == 0)]
    e = list(range(0, min(20, s.K), 2)) + idle + [ROOT_OB, 2 % s.K]
    return np.random.default_rng(s.seed + 1).permutation(np.array(e, dtype=np.int32))


def check_polygons_release(s):
    """scene P: the release burst after the union of the first 20 rows is blocked, at DELTA and at DELTA + 2^-30, against
    remove_obstacle_edges under the burst's flags; then unblock=True: a second call finds nothing left of those rows"""
    from rrtqx_3d_amd.context import Context
    out = {"rows": 0, "ids": 0}
    entries = polygon_release_entries(s)
    with Context(3) as ctx:
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, kinds=s.kinds, active=s.active)
        assert ctx.graph_edges_append(s.es, s.ee) == 0
        for name, d, blocked in (("DELTA", s.delta, s.blocked), ("DELTA + 2^-30", s.delta_up, s.blocked_up)):
            ctx.graph_edges_unblock(np.arange(len(s.es), dtype=np.int32))
            ctx.graph_edges_block(blocked)
            dist = np.ones(len(s.es))
            dist[blocked] = np.inf
            want = release_rows_reference(s, entries, dist, d, dubins=False)
            rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, s.rr, d, cap=8))
            for j, p in enumerate(entries):
                assert np.array_equal(rows[j], want[j]), f"scene {s.seed}: release row {j} (position {p}) at {name} differs"
            out["rows"] += len(rows); out["ids"] += sum(len(r) for r in rows)
        rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, s.rr, s.delta_up, unblock=True))
        assert all(np.array_equal(a, b) for a, b in zip(rows, want))
        assert len(ctx.obstacle_release_polygon_batch(entries, s.rr, s.delta_up)[1]) == 0
    return out


def check_dubins_release(s):
    """scene D: the rows of the first six positions blocked, then the release burst of four of them, the position not in
    use and a repeat, at DELTA and DELTA + 2^-30, against remove_obstacle_edges(dubins=True) under the burst's flags"""
    from rrtqx_3d_amd.context import Context
    out = {"rows": 0, "ids": 0}
    entries = np.array([1, 0, s.m - 2, 5, 2, 1], dtype=np.int32)
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(s.pts)
        ctx.polygons_set(s.polys, kinds=s.kinds, active=s.active)
        assert ctx.graph_edges_append(s.es, s.ee) == 0
        cost, _ = ctx.dubins_steer(s.pts[s.es], s.pts[s.ee], s.r_min)
        ctx.graph_edges_set_dist(0, cost)
        for name, d, base in (("DELTA", s.delta, s.rows), ("DELTA + 2^-30", s.delta_up, s.rows_up)):
            blocked = np.unique(np.concatenate(base[:6] + [np.zeros(0, np.int32)])).astype(np.int32)
            ctx.graph_edges_unblock(np.arange(len(s.es), dtype=np.int32))
            ctx.graph_edges_block(blocked)
            dist = cost.copy()
            dist[blocked] = np.inf
            want = release_rows_reference(s, entries, dist, d, dubins=True, r_min=s.r_min)
            rows = _rows_of(*ctx.obstacle_release_polygon_batch(entries, s.rr, d, r_min=s.r_min, cap=8))
            for j, p in enumerate(entries):
                assert np.array_equal(rows[j], want[j]), f"scene {s.seed}: Dubins release row {j} (position {p}) at {name} differs"
            out["rows"] += len(rows); out["ids"] += sum(len(r) for r in rows)
    return out


# ---- the soak -------------------------------------------------------------------------------------------------------------
def scene(sc):
    """soak scene sc: span, node count, K and RR drawn per scene; S, P and D (every third scene with a planted root)
    built with the oracle, compared through the C-ABI bit for bit; returns counts"""
    rng = np.random.default_rng(410_000 + sc)
    out = {}
    rr = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
    span = int(rng.choice([3, 6]))
    K = int(rng.choice([7, 65, 70, 130]))
    s = sphere_scene(420_000 + sc, n_draw=int(rng.choice([300, 1500, 3000])), span=span, K=K, rr=rr)
    o = check_spheres(s, solve=(sc % 4 == 0))
    out["sphere_rows"], out["sphere_ids"] = o["rows"], o["ids"]
    span = int(rng.choice([4, 8]))
    K = int(rng.choice([7, 64, 70]))
    p = polygon_scene(430_000 + sc, n_draw=int(rng.choice([400, 1200, 2500])), span=span, K=K, rr=rr,
                      delta=1.25 - rr, n_other=K // 5)            # rr + delta = 1.25: the root's 3-4-5 triple stays exact
    o = check_polygons(p)
    out["polygon_rows"], out["polygon_ids"] = o["rows"], o["ids"]
    o = check_polygons_release(p)
    out["polygon_release_rows"], out["polygon_release_ids"] = o["rows"], o["ids"]
    d = dubins_scene(440_000 + sc, root_planted=(sc % 3 == 0), n_draw=int(rng.choice([100, 300])), span=int(rng.choice([4, 6])),
                     rr=rr)
    o = check_dubins(d)
    out["dubins_rows"], out["dubins_ids"] = o["rows"], o["ids"]
    o = check_dubins_release(d)
    out["dubins_release_rows"], out["dubins_release_ids"] = o["rows"], o["ids"]
    return out


if __name__ == "__main__":
    n_scen = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    t0 = time.time()
    tot = {}
    for sc in range(n_scen):
        o = scene(sc)
        for k in o:
            tot[k] = tot.get(k, 0) + o[k]
        print(f"{sc + 1} scenes ok, {tot}, {time.time() - t0:.0f} s", flush=True)
    print("SOAK OK", n_scen, tot)
