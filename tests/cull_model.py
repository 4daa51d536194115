"""numpy restatement of rrtx_graph_edges_cull / rrtx_graph_edges_compact (include/rrtx.h), and the scenes their tests
share.  No test in this file; nothing here reads a device.

The rule: a mirrored edge is a current out-edge of its start node iff start < end (node indices are insertion order, and
extend() alone makes edges: new -> neighbour is the new node's initial out-neighbour, neighbour -> new the older node's
current one).  cullCurrentNeighbors(node, ball) (R/DRRT_Q.jl:2388-2403) for a set of nodes culls every edge that is not
yet culled, starts at a listed node, has start < end and dist > ball -- IEEE: NaN stays, dist == ball stays, +Inf goes --
and leaves it with dist = distOriginal = +Inf.  Compaction removes the culled edges; survivors keep their order."""
import math

import numpy as np

INF = float("inf")
LO, HI = -20.0, 20.0
DELTA = 8.0


def ball(n, ball_constant, delta=DELTA, d=3):
    """the shrinking ball at tree size n: min(delta, ball_constant (ln(1 + n) / n)^(1/d))"""
    return min(delta, ball_constant * (math.log(1 + n) / n) ** (1.0 / d))


def pair_dist(pts, s, e):
    """SimpleEdge cost as the device forms it: the squares summed left to right, one square root"""
    d = pts[s] - pts[e]
    acc = d[:, 0] * d[:, 0]
    for k in range(1, pts.shape[1]):
        acc = acc + d[:, k] * d[:, k]
    return np.sqrt(acc)


def growth_scene(n=2000, seed=5, ball_constant=30.0):
    """n uniform nodes in [LO, HI]^3, node 0 the root; i <-> j (i < j) linked when |p_i - p_j| < ball(j), as a tree grown
    one node at a time links them.  Edge order is extend()'s: for j ascending and its neighbours i ascending, the out-edge
    j -> i (initial), then the in-edge i -> j (current).  Returns (pts, start, end, dist)."""
    pts = np.random.default_rng(seed).uniform(LO, HI, (n, 3))
    s, e = [], []
    for j in range(1, n):
        i = np.arange(j)
        near = i[pair_dist(pts, i, np.full(j, j)) < ball(j, ball_constant)]
        pair = np.empty(2 * len(near), dtype=np.int32)
        pair[0::2], pair[1::2] = j, near
        s.append(pair)
        pair = np.empty(2 * len(near), dtype=np.int32)
        pair[0::2], pair[1::2] = near, j
        e.append(pair)
    s, e = np.concatenate(s), np.concatenate(e)
    return pts, s, e, pair_dist(pts, s, e)


def line_nodes(n=4):
    """nodes on a line at integer coordinates, so that an edge's cost is its index distance"""
    pts = np.zeros((n, 3))
    pts[:, 0] = np.arange(n)
    return pts


PATTERNS = ("none", "all", "every other", "first", "last", "runs")


def line_pattern(ne, pattern):
    """(start, end, culled) of ne edges over line_nodes whose culled set at ball = 1 is the named pattern: a culled edge is
    0 -> 2 (cost 2, current), a kept one alternates between 2 -> 0 (cost 2, initial), 0 -> 1 (cost 1 = ball) and
    1 -> 1 (a self loop)"""
    i = np.arange(ne)
    if pattern == "none":
        c = np.zeros(ne, dtype=bool)
    elif pattern == "all":
        c = np.ones(ne, dtype=bool)
    elif pattern == "every other":
        c = i % 2 == 0
    elif pattern == "first":
        c = i == 0
    elif pattern == "last":
        c = i == ne - 1
    elif pattern == "runs":                      # 100 edges from 50 before every multiple of 256
        c = ((i + 50) % 256) < 100
        c &= i + 50 >= 256
    else:
        raise ValueError(pattern)
    kept = np.array([[2, 0], [0, 1], [1, 1]], dtype=np.int32)[i % 3]
    s = np.where(c, 0, kept[:, 0]).astype(np.int32)
    e = np.where(c, 2, kept[:, 1]).astype(np.int32)
    return s, e, c


class CullModel:
    """The five columns the device keeps per edge, plus the pending touched mark"""

    def __init__(self, pts, start, end, dist=None):
        self.pts = np.ascontiguousarray(pts, dtype=np.float64)
        self.start = np.asarray(start, dtype=np.int32).copy()
        self.end = np.asarray(end, dtype=np.int32).copy()
        self.dist = (pair_dist(self.pts, self.start, self.end) if dist is None else np.asarray(dist, dtype=np.float64)).copy()
        self.dist0 = self.dist.copy()
        self.culled = np.zeros(len(self.start), dtype=np.uint8)

    @property
    def ne(self):
        return len(self.start)

    def append(self, start, end, dist=None):
        start, end = np.asarray(start, dtype=np.int32), np.asarray(end, dtype=np.int32)
        w = pair_dist(self.pts, start, end) if dist is None else np.asarray(dist, dtype=np.float64)
        self.start, self.end = np.concatenate([self.start, start]), np.concatenate([self.end, end])
        self.dist, self.dist0 = np.concatenate([self.dist, w]), np.concatenate([self.dist0, w])
        self.culled = np.concatenate([self.culled, np.zeros(len(start), dtype=np.uint8)])

    def set_dist(self, first, w):
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        self.dist[first:first + len(w)] = w
        self.dist0[first:first + len(w)] = w

    def block(self, ids):
        self.dist[np.asarray(ids, dtype=np.int64)] = INF

    def would_cull(self, ball_, nodes=None):
        """ids the rule culls now, ascending"""
        listed = np.ones(self.ne, dtype=bool) if nodes is None else np.isin(self.start, np.asarray(nodes))
        with np.errstate(invalid="ignore"):
            beyond = self.dist > ball_                       # IEEE: False for NaN, True for +Inf
        return np.flatnonzero((self.culled == 0) & listed & (self.start < self.end) & beyond).astype(np.int32)

    def cull(self, ball_, nodes=None):
        ids = self.would_cull(ball_, nodes)
        self.dist[ids] = INF
        self.dist0[ids] = INF
        self.culled[ids] = 1
        return ids

    def compact(self):
        """(remap, n_removed): remap[old] = new id, -1 for a removed edge; the columns shrink in place"""
        keep = self.culled == 0
        remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        self.start, self.end = self.start[keep], self.end[keep]
        self.dist, self.dist0 = self.dist[keep], self.dist0[keep]
        self.culled = self.culled[keep]
        return remap, int((~keep).sum())

    def columns(self):
        return self.start, self.end, self.dist, self.dist0
