"""A host model of what the device mirror of the planner's edges must hold after every C-ABI call (numpy only, no test
in this file), and Scene, the generator of nodes, edges and spheres the two sphere-burst test files share.  One entry per edge id: start, end, dist (edge.dist), dist0 (edge.distOriginal); the sphere table as the
context holds it (cxyzr, active); the node positions.  The methods carry the names of the Context methods and change
the model the way include/rrtx.h says the call changes the mirror; nothing is ever read back from a device.  The
oracle helpers give what a sweep, a release or a cost solve over the model's current state must return: rows from
oracle.sweep_edges_batch around the kd-tree's range query (the root's <=), exactly as Scene below forms them for
test_gpu_obstacle_sweep_batch.py / test_gpu_obstacle_release_batch.py, and rrtLMC from _oracle_solve of
test_gpu_graph_cost.py."""
import numpy as np

from rrtqx_3d_amd.context import Context
from test_gpu_graph_cost import _edge_dist, _oracle_solve

INF = float("inf")
RR, DELTA = 0.5, 8.0


class Scene:
    """The generator of test_obstacle_sweep_matches_oracle with K spheres (seed n + K).  The oracle's tree and sphere
    list are built once; sweep rows are computed once per (position, range), release rows once per (leaving set,
    position, range, blocked ids)."""

    def __init__(self, oracle, n, K, inactive=()):
        rng = np.random.default_rng(n + K)
        self.n, self.K, self.oracle = n, K, oracle
        self.pts = pts = rng.uniform(-30, 30, (n, 3))
        es = np.repeat(np.arange(n), 7)
        ee = (es + rng.integers(1, 50, len(es))) % n
        ee[::7] = rng.integers(0, n, n)                    # long edges too
        es[:5], ee[:5] = 0, [1, 2, 3, 4, 5]                # out-edges of the root
        ee[5] = es[5]                                      # a zero-length edge
        self.es, self.ee = es.astype(np.int32), ee.astype(np.int32)
        sph = np.concatenate([rng.uniform(-25, 25, (K, 3)), rng.uniform(1.0, 6.0, (K, 1))], 1)
        sph[3, :3] = pts[0] + [2.0, 0.0, 0.0]              # an obstacle right at the root
        sph[K - 1] = (29.5, 29.5, -29.5, 0.05)             # a tiny one in a corner
        self.sph = sph
        self.active = np.ones(K, dtype=np.uint8)
        self.active[list(inactive)] = 0
        self.search = RR + DELTA + sph[:, 3]
        self.tree = oracle.KDTree(3)
        self.tree.insert_many(pts)
        self.osph = oracle.make_spheres(sph, self.active)
        self._masks, self._rows, self._release_rows = {}, {}, {}

    def in_range(self, pos, search_range):
        key = (int(pos), float(search_range))
        if key not in self._masks:
            mask = np.zeros(self.n, dtype=np.uint8)
            mask[self.tree.within_range(float(search_range), self.sph[pos, :3])[0]] = 1
            self._masks[key] = mask
        return self._masks[key]

    def stay(self, leaving):
        s = self.active.copy()
        s[np.asarray(leaving, dtype=np.int64)] = 0
        return s

    def row(self, pos, search_range, es=None, ee=None):
        """the oracle's sweep of sphere `pos` with this range (over another mirror of the same nodes when given)"""
        key = (int(pos), float(search_range), None if es is None else id(es))
        if key not in self._rows:
            ids = self.oracle.sweep_edges_batch(self.pts, self.es if es is None else es, self.ee if ee is None else ee,
                                                self.in_range(pos, search_range), self.osph, int(pos), RR)
            self._rows[key] = np.asarray(ids, dtype=np.int32)
        return self._rows[key]

    def sweep_row(self, pos, search_range, es=None, ee=None):
        """addNewObstacle's loop for sphere `pos` taken as in use, whatever its flag says (oracle)"""
        a = np.zeros(self.K, dtype=np.uint8)
        a[pos] = 1
        ids = self.oracle.sweep_edges_batch(self.pts, self.es if es is None else es, self.ee if ee is None else ee,
                                            self.in_range(pos, search_range), self.oracle.make_spheres(self.sph, a),
                                            int(pos), RR)
        return np.asarray(ids, dtype=np.int32)

    def release_row(self, leaving, pos, search_range, dist_host, es=None, ee=None):
        """the reference for one row: the oracle alone, the stay flags with position `pos` set to 1"""
        key = (tuple(sorted(set(int(p) for p in leaving))), int(pos), float(search_range),
               np.flatnonzero(np.isinf(dist_host)).tobytes(), len(dist_host))
        if key not in self._release_rows:
            a = self.stay(leaving)
            a[pos] = 1
            ids = self.oracle.sweep_edges_batch(self.pts, self.es if es is None else es, self.ee if ee is None else ee,
                                                self.in_range(pos, search_range), self.oracle.make_spheres(self.sph, a),
                                                int(pos), RR, remove=True, dist=dist_host)
            self._release_rows[key] = np.asarray(ids, dtype=np.int32)
        return self._release_rows[key]

    def context(self, es=None, ee=None):
        ctx = Context(3)
        ctx.nodes_append(self.pts)
        ctx.spheres_set(self.sph, self.active)
        assert ctx.graph_edges_append(self.es if es is None else es, self.ee if ee is None else ee) == 0
        return ctx


class MirrorModel:
    def __init__(self, oracle, dim=3):
        self.oracle, self.dim = oracle, dim
        self.pts = np.zeros((0, dim))
        self.tree = oracle.KDTree(dim)
        self.start = np.zeros(0, dtype=np.int32)
        self.end = np.zeros(0, dtype=np.int32)
        self.dist = np.zeros(0)
        self.dist0 = np.zeros(0)
        self.cxyzr = np.zeros((0, 4))
        self.active = np.zeros(0, dtype=np.uint8)

    # ---- the calls ----------------------------------------------------------------------------------------------
    def nodes_append(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, self.dim)
        self.pts = np.concatenate([self.pts, pts])
        self.tree.insert_many(pts)                       # the reference's incremental tree: node 0 stays its root

    def append(self, s, e):
        s, e = np.asarray(s, dtype=np.int32), np.asarray(e, dtype=np.int32)
        assert s.shape == e.shape and (len(s) == 0 or max(s.max(), e.max()) < len(self.pts))
        first = len(self.start)
        w = _edge_dist(self.pts, s, e)
        self.start, self.end = np.concatenate([self.start, s]), np.concatenate([self.end, e])
        self.dist, self.dist0 = np.concatenate([self.dist, w]), np.concatenate([self.dist0, w])
        return first

    def set_dist(self, first, w):
        w = np.asarray(w, dtype=np.float64)
        assert 0 <= first and first + len(w) <= len(self.dist)
        self.dist[first:first + len(w)] = w
        self.dist0[first:first + len(w)] = w

    def block(self, ids):
        self.dist[np.asarray(ids, dtype=np.int64)] = INF

    def unblock(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self.dist[ids] = self.dist0[ids]

    def clear(self):
        self.start, self.end = self.start[:0], self.end[:0]
        self.dist, self.dist0 = self.dist[:0], self.dist0[:0]

    def spheres_set(self, cxyzr, active=None):
        self.cxyzr = np.array(cxyzr, dtype=np.float64).reshape(-1, 4)
        m = len(self.cxyzr)
        self.active = np.ones(m, dtype=np.uint8) if active is None else (np.asarray(active) != 0).astype(np.uint8)
        assert len(self.active) == m

    def obstacle_update(self, which, radius, active):
        self.cxyzr[which, 3] = radius
        self.active[which] = 1 if active else 0

    # ---- what the device has to return --------------------------------------------------------------------------
    @property
    def ne(self):
        return len(self.start)

    @property
    def blocked(self):
        return np.flatnonzero(np.isinf(self.dist)).astype(np.int32)

    def in_range(self, j, search_range):
        mask = np.zeros(len(self.pts), dtype=np.uint8)
        mask[self.tree.within_range(float(search_range), self.cxyzr[j, :3])[0]] = 1
        return mask

    def hits(self, j, search_range, rr):
        """the edges that start in range of sphere j and collide with it, whatever its flag and their cost"""
        a = np.zeros(len(self.cxyzr), dtype=np.uint8)
        a[j] = 1
        return self.oracle.sweep_edges_batch(self.pts, self.start, self.end, self.in_range(j, search_range),
                                             self.oracle.make_spheres(self.cxyzr, a), int(j), rr)

    def sweep_row(self, j, search_range, rr):
        """rrtx_obstacle_sweep(j, search_range, rr): addNewObstacle's loop; a sphere that is not in use hits nothing"""
        if self.ne == 0 or not self.active[j]:
            return np.zeros(0, dtype=np.int32)
        return self.hits(j, search_range, rr)

    def release_row(self, j, search_range, rr, leaving):
        """row of sphere j in rrtx_obstacle_release_batch(leaving, ...): blocked, in range of j and hitting it (its own
        flag is not read), hitting no sphere that is in use and not in `leaving`"""
        if self.ne == 0:
            return np.zeros(0, dtype=np.int32)
        a = self.active.copy()
        a[np.asarray(leaving, dtype=np.int64)] = 0
        a[j] = 1
        return self.oracle.sweep_edges_batch(self.pts, self.start, self.end, self.in_range(j, search_range),
                                             self.oracle.make_spheres(self.cxyzr, a), int(j), rr, remove=True,
                                             dist=self.dist)

    def packed_position(self):
        """position of every sphere among the ones in use, table order (-1: not in use)"""
        return np.where(self.active != 0, np.cumsum(self.active != 0) - 1, -1)

    def hit_matrix_rows(self, ids, rr):
        """for each edge id, the table positions of the spheres (in use or not) the edge collides with"""
        out = []
        p0, p1 = self.pts[self.start[ids]], self.pts[self.end[ids]]
        cols = []
        for j in range(len(self.cxyzr)):
            a = np.zeros(len(self.cxyzr), dtype=np.uint8)
            a[j] = 1
            hit, _ = self.oracle.edges_check_spheres(*self.oracle.make_spheres(self.cxyzr, a), p0, p1, rr)
            cols.append(np.asarray(hit) != 0)
        hm = np.stack(cols, 1) if cols else np.zeros((len(ids), 0), dtype=bool)
        for r in hm:
            out.append(np.flatnonzero(r))
        return out, hm

    def solve(self, root):
        """(rrtLMC, parent edge by the reference's visiting order) of the fixed point over the current costs"""
        lmc, par = _oracle_solve(self.oracle, len(self.pts), self.start, self.end, self.dist, root)
        return lmc, par
