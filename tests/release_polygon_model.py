"""What rrtx_obstacle_release_polygon_batch must return, from the oracle alone (no device): the rows of a burst of
expiring polygon obstacles as sweep_edges_batch(remove=True) in C gives them under the burst's flags, the reference's
one-by-one sequence over the same mirror, and the rand_Disc_3 scene of test_gpu_obstacle_sweep_polygon.py both are
judged on.  Shared by test_oracle_release_polygon_sequence.py and test_gpu_obstacle_release_polygon_batch.py."""
import json
import os
import types

import numpy as np

RR, DELTA = 0.5, 8.0                               # those of test_gpu_obstacle_sweep_polygon.py
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def graph(tree, pts, r, rng, n_long=200):
    """test_gpu_obstacle_sweep_polygon._graph, draw for draw (that module needs the device library to import)"""
    es, ee = [], []
    for i in range(len(pts)):
        idx, _ = tree.within_range(r, pts[i])
        for j in np.sort(idx):
            if j != i:
                es.append(i); ee.append(int(j))
    es += rng.integers(0, len(pts), n_long).tolist()
    ee += rng.integers(0, len(pts), n_long).tolist()
    es += [0, 0, 0, 7]
    ee += [1, 2, 3, 7]
    return np.array(es, dtype=np.int32), np.array(ee, dtype=np.int32)


class Scene(types.SimpleNamespace):
    """nodes pts in tree, mirror es -> ee, polygon list (polys, kinds, paths, active); edge = oracle.EDGE_*"""

    def polygon_set(self, oracle, active=None):
        return oracle.PolygonSet(self.polys, kinds=self.kinds, paths=self.paths, active=self.active if active is None else active)

    def mask(self, oracle, p):
        """in_conflict per node for list position p (findPointsInConflictWithObstacle; the flag is not read)"""
        if p not in self._masks:
            m = np.zeros(len(self.pts), dtype=np.uint8)
            m[oracle.points_in_conflict_polygon(self.tree, self.ps, int(p), RR, self.delta, self.has_time, self.edge != oracle.EDGE_SIMPLE)] = 1
            self._masks[p] = m
        return self._masks[p]

    def add_rows(self, oracle, positions, ne=None):
        """mode 0 (addNewObstacle's loop) of every position, under the scene's own flags, over the first ne edges"""
        return {int(p): oracle.sweep_edges_batch(self.pts, self.es[:ne], self.ee[:ne], self.mask(oracle, int(p)), self.ps, int(p), RR,
                                                 edge=self.edge, r_min=self.r_min) for p in positions}

    def burst_rows(self, oracle, entries, dist, active=None):
        """the rows of a release burst: entry j as removeObstacle's loop sees it when the OTHER listed positions are not in
        use -- what stays (in use and not listed) is the same for all rows, the entry itself keeps its own flag"""
        active = np.array(self.active if active is None else active, dtype=np.uint8)
        flags = active.copy()
        flags[np.asarray(entries, dtype=np.int64)] = 0
        ps = self.polygon_set(oracle, flags)
        ne = len(dist)
        rows = {}
        for p in sorted(set(int(q) for q in entries)):
            ps.arr[p].unused = 0 if active[p] else 1
            rows[p] = oracle.sweep_edges_batch(self.pts, self.es[:ne], self.ee[:ne], self.mask(oracle, p), ps, p, RR, edge=self.edge,
                                               remove=True, dist=dist, r_min=self.r_min)
            ps.arr[p].unused = 1
        return [rows[int(p)] for p in entries]

    def sequence_rows(self, oracle, entries, dist, dist0):
        """the reference's order: remove A, unblock its row, mark A unused, remove B, ...; returns the rows"""
        dist = np.array(dist, dtype=np.float64)
        flags = np.array(self.active, dtype=np.uint8).copy()
        ps = self.polygon_set(oracle, flags)
        ne = len(dist)
        rows = []
        for p in entries:
            p = int(p)
            row = oracle.sweep_edges_batch(self.pts, self.es[:ne], self.ee[:ne], self.mask(oracle, p), ps, p, RR, edge=self.edge,
                                           remove=True, dist=dist, r_min=self.r_min)
            dist[row] = dist0[row]
            ps.arr[p].unused = 1
            rows.append(row)
        return rows

    def candidates(self, oracle, entries, dist, active=None):
        """last_sweep_candidates of a release: per group of 64 entries the BLOCKED mirrored edges that start at a node some
        in-use obstacle of the group is in conflict with, summed over the groups; also the per-group counts"""
        active = self.active if active is None else active
        ne = len(dist)
        per_group = []
        for g0 in range(0, len(entries), 64):
            nodes = np.zeros(len(self.pts), dtype=bool)
            for p in entries[g0:g0 + 64]:
                if active[p]:
                    nodes |= self.mask(oracle, int(p)) != 0
            per_group.append(int((nodes[self.es[:ne]] & (dist == np.inf)).sum()))
        return sum(per_group), per_group


def make_scene(oracle, pts, tree, es, ee, polys, active, kinds=None, paths=None, edge=None, r_min=0.0, has_time=False, delta=DELTA):
    s = Scene(pts=pts, tree=tree, es=es, ee=ee, polys=polys, m=len(polys), active=np.asarray(active, dtype=np.uint8), kinds=kinds,
              paths=paths, edge=oracle.EDGE_SIMPLE if edge is None else edge, r_min=r_min, has_time=has_time, delta=delta, _masks={})
    s.ps = s.polygon_set(oracle)
    return s


def simple_scene(oracle):
    """SimpleEdge, the reference's rand_Disc_3 polygons: the scene of test_simple_edges_discoverable_polygons (same seed
    and sizes), positions 4 and 30 not in use"""
    polys = [np.array(p) for p in json.load(open(os.path.join(G, "env_inputs.json")))["rand_Disc_3_polygons"]]
    m = len(polys)
    rng = np.random.default_rng(5)
    n = 2500
    pts = np.c_[rng.uniform(-20, 20, (n, 2)), np.zeros(n)]
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    es, ee = graph(tree, pts, 2.5, rng)
    active = np.ones(m, dtype=np.uint8)
    active[[4, 30]] = 0
    s = make_scene(oracle, pts, tree, es, ee, polys, active)
    s.length = np.sqrt(((pts[es] - pts[ee]) ** 2).sum(axis=1))
    return s
