"""ctypes loader for the CPU oracle (oracle/rrtx_oracle.c).

TEST INFRASTRUCTURE ONLY: import this from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg -- never from rrtqx_3d_amd/ (the product path).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "librrtx_oracle.so")
# the same source with glibc's sin / cos / atan2 / acos on the Dubins paths (-DORC_LIBM_TRIG): CPU cross-check only
_LIBM_PATH = os.path.join(_HERE, "_build", "librrtx_oracle_libm.so")

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)


class Sphere(C.Structure):
    _fields_ = [("c", C.c_double * 3), ("radius", C.c_double), ("life_span", C.c_double),
                ("unused", C.c_int32), ("pad", C.c_int32)]


class Polygon(C.Structure):
    _fields_ = [("kind", C.c_int32), ("nverts", C.c_int32), ("verts", c_double_p),
                ("cx", C.c_double), ("cy", C.c_double), ("radius", C.c_double),
                ("life_span", C.c_double), ("unused", C.c_int32), ("npath", C.c_int32),
                ("path", c_double_p)]


def build(force: bool = False) -> str:
    """Compile the oracle with gcc (seconds). Returns the .so path."""
    src = os.path.join(_HERE, "rrtx_oracle.c")
    src2 = os.path.join(_HERE, "rrtx_oracle_graph.c")
    hdr = os.path.join(_HERE, "rrtx_oracle.h")
    dm = os.path.join(_HERE, "..", "include", "rrtx_detmath.h")
    stale = (not os.path.exists(_LIB_PATH) or not os.path.exists(_LIBM_PATH)
             or any(os.path.exists(p) and os.path.getmtime(p) > os.path.getmtime(_LIB_PATH) for p in (src, src2, hdr, dm)))
    if force or stale:
        subprocess.run(["make", "-C", _HERE, "-s"], check=True)
    return _LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    build()
    L = C.CDLL(_LIB_PATH)
    L.orc_euclid.restype = C.c_double
    L.orc_euclid.argtypes = [c_double_p, c_double_p, C.c_int]
    L.orc_ball_radius.restype = C.c_double
    L.orc_ball_radius.argtypes = [C.c_double, C.c_double, C.c_int64, C.c_int]
    L.orc_kd_create.restype = C.c_void_p
    L.orc_kd_create.argtypes = [C.c_int]
    L.orc_kd_destroy.argtypes = [C.c_void_p]
    L.orc_kd_set_wraps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), c_double_p]
    L.orc_kd_insert.restype = C.c_int64
    L.orc_kd_insert.argtypes = [C.c_void_p, c_double_p]
    L.orc_kd_size.restype = C.c_int64
    L.orc_kd_size.argtypes = [C.c_void_p]
    L.orc_kd_depth.restype = C.c_int64
    L.orc_kd_depth.argtypes = [C.c_void_p]
    L.orc_kd_nearest.argtypes = [C.c_void_p, c_double_p, c_int64_p, c_double_p]
    L.orc_kd_nearest_naive.argtypes = [C.c_void_p, c_double_p, c_int64_p, c_double_p]
    L.orc_kd_find_within_range.restype = C.c_void_p
    L.orc_kd_find_within_range.argtypes = [C.c_void_p, C.c_double, c_double_p]
    L.orc_kd_find_more_within_range.argtypes = [C.c_void_p, C.c_double, c_double_p, C.c_void_p]
    L.orc_list_length.restype = C.c_int64
    L.orc_list_length.argtypes = [C.c_void_p]
    L.orc_list_read.restype = C.c_int64
    L.orc_list_read.argtypes = [C.c_void_p, C.c_int64, c_int32_p, c_double_p]
    L.orc_kd_empty_range_list.argtypes = [C.c_void_p, C.c_void_p]
    for f in (L.orc_kd_knearest, L.orc_kd_knearest_naive):
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_int64, c_double_p, C.c_int64, c_int32_p, c_double_p]
    L.orc_range_naive.restype = C.c_int64
    L.orc_range_naive.argtypes = [C.c_void_p, C.c_double, c_double_p, C.c_int64, c_int32_p, c_double_p]
    L.orc_ghost_points.restype = C.c_int
    L.orc_ghost_points.argtypes = [C.c_void_p, c_double_p, C.c_double, C.c_int, c_double_p]
    L.orc_distance_point_to_segment3.restype = C.c_double
    L.orc_distance_point_to_segment3.argtypes = [c_double_p] * 3
    L.orc_edge_check_sphere.restype = C.c_int
    L.orc_edge_check_sphere.argtypes = [C.POINTER(Sphere), c_double_p, c_double_p, C.c_double]
    L.orc_edge_check_spheres.restype = C.c_int
    L.orc_edge_check_spheres.argtypes = [C.POINTER(Sphere), C.c_int, c_double_p, c_double_p, C.c_double, c_int32_p]
    L.orc_point_check_spheres.restype = C.c_int
    L.orc_point_check_spheres.argtypes = [C.POINTER(Sphere), C.c_int, c_double_p, C.c_double, C.c_int, c_double_p]
    L.orc_polygon_ctor.argtypes = [c_double_p, C.c_int, c_double_p, c_double_p, c_double_p]
    L.orc_dist_sqrd_point_to_segment.restype = C.c_double
    L.orc_dist_sqrd_point_to_segment.argtypes = [c_double_p] * 3
    L.orc_segment_dist_sqrd.restype = C.c_double
    L.orc_segment_dist_sqrd.argtypes = [c_double_p] * 4
    L.orc_point_in_polygon.restype = C.c_int
    L.orc_point_in_polygon.argtypes = [c_double_p, c_double_p, C.c_int]
    L.orc_dist_to_polygon_sqrd.restype = C.c_double
    L.orc_dist_to_polygon_sqrd.argtypes = [c_double_p, c_double_p, C.c_int]
    L.orc_edge_check_polygon.restype = C.c_int
    L.orc_edge_check_polygon.argtypes = [C.POINTER(Polygon), c_double_p, c_double_p, C.c_double]
    L.orc_edge_check_polygons.restype = C.c_int
    L.orc_edge_check_polygons.argtypes = [C.POINTER(Polygon), C.c_int, c_double_p, c_double_p, C.c_double, c_int32_p]
    L.orc_point_check_polygons.restype = C.c_int
    L.orc_point_check_polygons.argtypes = [C.POINTER(Polygon), C.c_int, c_double_p, C.c_double, c_double_p]
    L.orc_dubins_steer.argtypes = [c_double_p, c_double_p, C.c_double, c_double_p, C.c_char_p,
                                   c_double_p, C.c_int, C.POINTER(C.c_int)]
    L.orc_dubins_edge_check_polygons.restype = C.c_int
    L.orc_dubins_edge_check_polygons.argtypes = [C.POINTER(Polygon), C.c_int, c_double_p, c_double_p,
                                                 c_double_p, C.c_int, C.c_double, C.c_double, c_int32_p]
    for f in (L.orc_dubins_steer_time, L.orc_dubins_steer_time_pw):
        f.argtypes = [c_double_p, c_double_p, C.c_double, c_double_p, c_double_p, c_double_p,
                      C.c_char_p, c_double_p, C.c_int, C.POINTER(C.c_int)]
    L.orc_find_points_in_conflict_polygon.restype = C.c_void_p
    L.orc_find_points_in_conflict_polygon.argtypes = [C.c_void_p, C.POINTER(Polygon), C.c_double, C.c_double, C.c_int, C.c_int]
    L.orc_dm_eval.restype = C.c_int
    L.orc_dm_eval.argtypes = [C.c_int, c_double_p, c_double_p, C.c_int64, c_double_p]
    L.orc_dubins_valid_move_time.restype = C.c_int
    L.orc_dubins_valid_move_time.argtypes = [c_double_p, c_double_p, C.c_double, C.c_double, C.c_double]
    L.orc_dubins_edge_check_polygons_time.restype = C.c_int
    L.orc_dubins_edge_check_polygons_time.argtypes = [C.POINTER(Polygon), C.c_int, c_double_p, c_double_p,
                                                      c_double_p, C.c_int, C.c_double, C.c_double, c_int32_p]
    L.orc_graph_create.restype = C.c_void_p
    L.orc_graph_create.argtypes = [C.c_int64]
    L.orc_graph_destroy.argtypes = [C.c_void_p]
    L.orc_graph_add_edge.restype = C.c_int64
    L.orc_graph_add_edge.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_int, C.c_int]
    L.orc_graph_set_node.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double]
    L.orc_graph_set_move_goal.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    L.orc_graph_set_edge_dist.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    for f in (L.orc_graph_lmc, L.orc_graph_tree_cost):
        f.restype = C.c_double
        f.argtypes = [C.c_void_p, C.c_int64]
    L.orc_graph_parent_edge.restype = C.c_int64
    L.orc_graph_parent_edge.argtypes = [C.c_void_p, C.c_int64]
    L.orc_graph_queue_length.restype = C.c_int64
    L.orc_graph_queue_length.argtypes = [C.c_void_p]
    L.orc_graph_n_edges.restype = C.c_int64
    L.orc_graph_n_edges.argtypes = [C.c_void_p]
    L.orc_graph_verify_in_queue.argtypes = [C.c_void_p, C.c_int64]
    L.orc_graph_verify_in_os.argtypes = [C.c_void_p, C.c_int64]
    L.orc_graph_make_parent_of.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    L.orc_graph_reduce_inconsistency.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double]
    L.orc_graph_block_edge.argtypes = [C.c_void_p, C.c_int64]
    L.orc_graph_propagate_descendants.argtypes = [C.c_void_p]
    L.orc_graph_add_edges.restype = C.c_int64
    L.orc_graph_add_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]
    L.orc_graph_read.restype = None
    L.orc_graph_read.argtypes = [C.c_void_p] * 4
    L.orc_graph_block_edges.restype = None
    L.orc_graph_block_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.orc_sweep_edges_batch.restype = C.c_int
    L.orc_sweep_edges_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_double, C.c_double, C.c_void_p]
    L.orc_julia_range_len.restype = C.c_int64
    L.orc_julia_range_len.argtypes = [C.c_double] * 3
    L.orc_kd_insert_many.restype = None
    L.orc_kd_insert_many.argtypes = [C.c_void_p, c_double_p, C.c_int64]
    L.orc_extend_batch_spheres.restype = C.c_int64
    L.orc_extend_batch_spheres.argtypes = [C.c_void_p, C.POINTER(Sphere), C.c_int, c_double_p, C.c_int64,
                                           C.c_double, C.c_double, c_int64_p, c_int64_p, c_int64_p]
    L.orc_extend_batch_polygons.restype = C.c_int64
    L.orc_extend_batch_polygons.argtypes = [C.c_void_p, C.POINTER(Polygon), C.c_int, c_double_p, C.c_int64,
                                            C.c_double, C.c_double, c_int64_p, c_int64_p, c_int64_p]
    vp = C.c_void_p
    L.orc_range_batch.restype = C.c_int64
    L.orc_range_batch.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int64] + [vp] * 5
    L.orc_knearest_batch.restype = C.c_int
    L.orc_knearest_batch.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.orc_simple_candidates_batch.restype = C.c_int
    L.orc_simple_candidates_batch.argtypes = [vp, C.c_int64, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, vp, vp, C.c_int,
                                              C.c_double] + [vp] * 6
    L.orc_edges_check_batch.restype = None
    L.orc_edges_check_batch.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp, C.c_int, C.c_double, vp, vp]
    L.orc_points_check_batch.restype = None
    L.orc_points_check_batch.argtypes = [vp, C.c_int64, C.c_int, vp, vp, C.c_int, C.c_double, C.c_int, vp, vp]
    L.orc_dubins_edges_batch.restype = C.c_int
    L.orc_dubins_edges_batch.argtypes = [vp, vp, C.c_int64, C.c_double, C.c_double, C.POINTER(Polygon), C.c_int, C.c_int,
                                         C.c_int, C.c_double, C.c_double] + [vp] * 10
    L.orc_dubins_candidates_batch.restype = C.c_int
    L.orc_dubins_candidates_batch.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                              C.POINTER(Polygon), C.c_int, C.c_int, C.c_int, C.c_double,
                                              C.c_double] + [vp] * 6
    _lib = L
    return L


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def _vec(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))


def euclid(x, y) -> float:
    x, y = _vec(x), _vec(y)
    return lib().orc_euclid(_dp(x), _dp(y), len(x))


def ball_radius(delta: float, ball_constant: float, n: int, d: int) -> float:
    return lib().orc_ball_radius(delta, ball_constant, n, d)


class KDTree:
    """The reference's incremental kd-tree (R/kdTree_general.jl)."""

    def __init__(self, d: int, wraps=None, wrap_points=None):
        self.d = d
        self._h = lib().orc_kd_create(d)
        if wraps:
            w = (C.c_int * len(wraps))(*wraps)
            wp = (C.c_double * len(wraps))(*wrap_points)
            lib().orc_kd_set_wraps(self._h, len(wraps), w, wp)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().orc_kd_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def insert(self, pos) -> int:
        p = _vec(pos)
        assert len(p) == self.d
        return lib().orc_kd_insert(self._h, _dp(p))

    def insert_many(self, pts: np.ndarray):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        assert pts.ndim == 2 and pts.shape[1] == self.d
        lib().orc_kd_insert_many(self._h, _dp(pts), pts.shape[0])

    @property
    def size(self) -> int:
        return lib().orc_kd_size(self._h)

    def depth(self) -> int:
        return lib().orc_kd_depth(self._h)

    def nearest(self, q, naive: bool = False):
        q = _vec(q)
        idx = C.c_int64()
        dist = C.c_double()
        f = lib().orc_kd_nearest_naive if naive else lib().orc_kd_nearest
        f(self._h, _dp(q), C.byref(idx), C.byref(dist))
        return idx.value, dist.value

    def within_range(self, r: float, q, more=()):
        """kdFindWithinRange (+ kdFindMoreWithinRange for each extra (r, q) in `more`).
        Returns (idx, key) in list order (front first)."""
        q = _vec(q)
        L = lib()
        lst = L.orc_kd_find_within_range(self._h, r, _dp(q))
        for (r2, q2) in more:
            q2 = _vec(q2)
            L.orc_kd_find_more_within_range(self._h, r2, _dp(q2), lst)
        n = L.orc_list_length(lst)
        idx = np.empty(n, dtype=np.int32)
        key = np.empty(n, dtype=np.float64)
        L.orc_list_read(lst, n, idx.ctypes.data_as(c_int32_p), _dp(key))
        L.orc_kd_empty_range_list(self._h, lst)
        return idx, key

    def knearest(self, k: int, q, naive: bool = False):
        """kdFindKNearest / kdFindKNearestNaive: (idx, key) in heap order; raises where the
        reference does (wrapped space)."""
        q = _vec(q)
        f = lib().orc_kd_knearest_naive if naive else lib().orc_kd_knearest
        cap = max(int(k), 2) + 1
        idx = np.empty(cap, dtype=np.int32)
        key = np.empty(cap, dtype=np.float64)
        n = f(self._h, int(k), _dp(q), cap, idx.ctypes.data_as(c_int32_p), _dp(key))
        if n < 0:
            raise RuntimeError("knn search has not been implimented for wrapped space")
        return idx[:n].copy(), key[:n].copy()

    def range_naive(self, r: float, q):
        q = _vec(q)
        L = lib()
        n = L.orc_range_naive(self._h, r, _dp(q), 0, None, None)
        idx = np.empty(n, dtype=np.int32)
        key = np.empty(n, dtype=np.float64)
        L.orc_range_naive(self._h, r, _dp(q), n, idx.ctypes.data_as(c_int32_p), _dp(key))
        return idx, key

    def ghost_points(self, q, best_dist: float):
        q = _vec(q)
        out = np.empty((64, self.d), dtype=np.float64)
        n = lib().orc_ghost_points(self._h, _dp(q), best_dist, 64, _dp(out))
        return out[:n].copy()


def make_spheres(cxyzr: np.ndarray, active=None, life_span=None):
    cxyzr = np.asarray(cxyzr, dtype=np.float64).reshape(-1, 4)
    m = cxyzr.shape[0]
    arr = (Sphere * max(m, 1))()
    for i in range(m):
        arr[i].c[0], arr[i].c[1], arr[i].c[2] = cxyzr[i, 0], cxyzr[i, 1], cxyzr[i, 2]
        arr[i].radius = cxyzr[i, 3]
        arr[i].life_span = float("inf") if life_span is None else float(life_span[i])
        arr[i].unused = 0 if (active is None or active[i]) else 1
    return arr, m


def distance_point_to_segment3(c, p0, p1) -> float:
    c, p0, p1 = _vec(c), _vec(p0), _vec(p1)
    return lib().orc_distance_point_to_segment3(_dp(c), _dp(p0), _dp(p1))


def edge_check_spheres(spheres, m, p0, p1, robot_radius):
    p0, p1 = _vec(p0), _vec(p1)
    fh = C.c_int32()
    hit = lib().orc_edge_check_spheres(spheres, m, _dp(p0), _dp(p1), robot_radius, C.byref(fh))
    return bool(hit), fh.value


def edges_check_spheres(spheres, m, P0: np.ndarray, P1: np.ndarray, robot_radius: float):
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    n, d = P0.shape
    hit = np.zeros(n, dtype=np.uint8)
    first = np.full(n, -1, dtype=np.int32)
    f = lib().orc_edge_check_spheres
    fh = C.c_int32()
    b0, b1, st = P0.ctypes.data, P1.ctypes.data, d * 8
    for i in range(n):
        hit[i] = f(spheres, m, C.cast(b0 + i * st, c_double_p), C.cast(b1 + i * st, c_double_p),
                   robot_radius, C.byref(fh))
        first[i] = fh.value
    return hit, first


def point_check_spheres(spheres, m, p, robot_radius, quick=True):
    p = _vec(p)
    cl = C.c_double()
    r = lib().orc_point_check_spheres(spheres, m, _dp(p), robot_radius, 1 if quick else 0, C.byref(cl))
    return bool(r), cl.value


def points_check_spheres(spheres, m, P: np.ndarray, robot_radius, quick=True):
    P = np.ascontiguousarray(P, dtype=np.float64)
    n, d = P.shape
    unsafe = np.zeros(n, dtype=np.uint8)
    clr = np.zeros(n, dtype=np.float64)
    cl = C.c_double()
    f = lib().orc_point_check_spheres
    for i in range(n):
        unsafe[i] = f(spheres, m, C.cast(P.ctypes.data + i * d * 8, c_double_p), robot_radius,
                      1 if quick else 0, C.byref(cl))
        clr[i] = cl.value
    return unsafe, clr


def polygon_ctor(verts):
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 2))
    cx, cy, r = C.c_double(), C.c_double(), C.c_double()
    lib().orc_polygon_ctor(_dp(v), v.shape[0], C.byref(cx), C.byref(cy), C.byref(r))
    return cx.value, cy.value, r.value


class PolygonSet:
    """A list of polygon obstacles in list order: kind 3 (static), 1 (ball), 6 / 7 (moving along
    paths[i], rows of (dx, dy, t))."""

    def __init__(self, polys, kinds=None, active=None, paths=None):
        self.verts = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 2)) for p in polys]
        self.m = len(self.verts)
        self.arr = (Polygon * max(self.m, 1))()
        self.paths = [None] * self.m
        for i in range(self.m):
            if paths is not None and paths[i] is not None and len(paths[i]):
                self.paths[i] = np.ascontiguousarray(np.asarray(paths[i], dtype=np.float64).reshape(-1, 3))
                self.arr[i].npath = self.paths[i].shape[0]
                self.arr[i].path = _dp(self.paths[i])
        for i, v in enumerate(self.verts):
            cx, cy, r = polygon_ctor(v)
            a = self.arr[i]
            a.kind = 3 if kinds is None else int(kinds[i])
            a.nverts = v.shape[0]
            a.verts = _dp(v)
            a.cx, a.cy, a.radius = cx, cy, r
            a.life_span = float("inf")
            a.unused = 0 if (active is None or active[i]) else 1

    def centre_radius(self) -> np.ndarray:
        return np.array([[self.arr[i].cx, self.arr[i].cy, self.arr[i].radius] for i in range(self.m)],
                        dtype=np.float64).reshape(-1, 3)


def dist_sqrd_point_to_segment(pt, a, b) -> float:
    pt, a, b = _vec(pt), _vec(a), _vec(b)
    return lib().orc_dist_sqrd_point_to_segment(_dp(pt), _dp(a), _dp(b))


def segment_dist_sqrd(pa, pb, qa, qb) -> float:
    pa, pb, qa, qb = _vec(pa), _vec(pb), _vec(qa), _vec(qb)
    return lib().orc_segment_dist_sqrd(_dp(pa), _dp(pb), _dp(qa), _dp(qb))


def point_in_polygon(pt, verts) -> bool:
    pt = _vec(pt)
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 2))
    return bool(lib().orc_point_in_polygon(_dp(pt), _dp(v), v.shape[0]))


def edge_check_polygons(ps: PolygonSet, p0, p1, robot_radius):
    p0, p1 = _vec(p0), _vec(p1)
    fh = C.c_int32()
    hit = lib().orc_edge_check_polygons(ps.arr, ps.m, _dp(p0), _dp(p1), robot_radius, C.byref(fh))
    return bool(hit), fh.value


def edges_check_polygons(ps: PolygonSet, P0, P1, robot_radius):
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    n, d = P0.shape
    hit = np.zeros(n, dtype=np.uint8)
    first = np.full(n, -1, dtype=np.int32)
    fh = C.c_int32()
    f = lib().orc_edge_check_polygons
    for i in range(n):
        hit[i] = f(ps.arr, ps.m, C.cast(P0.ctypes.data + i * d * 8, c_double_p),
                   C.cast(P1.ctypes.data + i * d * 8, c_double_p), robot_radius, C.byref(fh))
        first[i] = fh.value
    return hit, first


def point_check_polygons(ps: PolygonSet, p, robot_radius):
    p = _vec(p)
    cl = C.c_double()
    r = lib().orc_point_check_polygons(ps.arr, ps.m, _dp(p), robot_radius, C.byref(cl))
    return bool(r), cl.value


def points_in_conflict_polygon(tree: "KDTree", ps: "PolygonSet", j: int, robot_radius: float, delta: float,
                               has_time: bool, has_theta: bool) -> np.ndarray:
    """findPointsInConflictWithObstacle(S, KD, ob::Obstacle, root) (R/DRRT.jl:3048-3125) for obstacle j of the
    list: the node indices of the range list in list order; raises where the reference does."""
    L = lib()
    lst = L.orc_find_points_in_conflict_polygon(tree._h, C.byref(ps.arr[j]), robot_radius, delta, int(has_time), int(has_theta))
    if not lst:
        raise RuntimeError("this type of obstacle not coded for this type of space")
    n = L.orc_list_length(lst)
    idx = np.empty(n, dtype=np.int32)
    key = np.empty(n, dtype=np.float64)
    L.orc_list_read(lst, n, idx.ctypes.data_as(c_int32_p), _dp(key))
    L.orc_kd_empty_range_list(tree._h, lst)
    return idx


def explicit_edge_check_obstacle(ps: "PolygonSet", j: int, a, b, robot_radius: float, dubins: bool, r_min: float = 0.0,
                                 has_time: bool = False, piecewise_time: bool = True) -> bool:
    """explicitEdgeCheck(S, edge, ob) against ONE obstacle of the list: SimpleEdge -> explicitEdgeCheck2D
    (R/DRRT_SimpleEdge_functions.jl:210-212 with the polygon ob), DubinsEdge -> the two-stage check
    (R/DRRT_DubinsEdge_functions.jl:750-774) on the edge's own trajectory."""
    a, b = _vec(a), _vec(b)
    one = C.byref(ps.arr[j])
    if not dubins:
        return bool(lib().orc_edge_check_polygon(one, _dp(a), _dp(b), robot_radius))
    fh = C.c_int32()
    if has_time:
        d, w, v, wd, tr = dubins_steer_time(a, b, r_min, piecewise=piecewise_time)
        if not np.isfinite(w) or len(tr) == 0:
            tr = np.zeros((0, 3))
        return bool(lib().orc_dubins_edge_check_polygons_time(one, 1, _dp(a), _dp(b), _dp(np.ascontiguousarray(tr)), len(tr),
                                                              robot_radius, r_min, C.byref(fh)))
    c, w, traj = dubins_steer(a, b, r_min)
    r = lib().orc_dubins_edge_check_polygons(one, 1, _dp(a), _dp(b), _dp(np.ascontiguousarray(traj)), len(traj), robot_radius,
                                             r_min, C.byref(fh))
    if r < 0:
        raise RuntimeError("Dubins edges against moving obstacles need the time-parameterised trajectory")
    return bool(r)


def add_new_obstacle_edges(tree: "KDTree", pts: np.ndarray, e_start, e_end, ps: "PolygonSet", j: int, robot_radius: float,
                           delta: float, dubins: bool, r_min: float = 0.0, has_time: bool = False) -> np.ndarray:
    """The edge loop of addNewObstacle (R/DRRT.jl:3127-3200) over a mirror of the planner's directed edges: every
    edge that STARTS at a node of findPointsInConflictWithObstacle's list (its out-neighbour edges and its parent
    edge) and for which explicitEdgeCheck(S, edge, ob) is true -- the edges the reference sets to dist = Inf.
    Ascending edge ids."""
    nodes = set(points_in_conflict_polygon(tree, ps, j, robot_radius, delta, has_time, dubins).tolist())
    out = []
    for e in range(len(e_start)):
        if int(e_start[e]) in nodes and explicit_edge_check_obstacle(ps, j, pts[e_start[e]], pts[e_end[e]], robot_radius, dubins,
                                                                     r_min, has_time):
            out.append(e)
    return np.array(out, dtype=np.int32)


def remove_obstacle_edges(tree: "KDTree", pts: np.ndarray, e_start, e_end, e_dist, ps: "PolygonSet", j: int,
                          robot_radius: float, delta: float, dubins: bool, r_min: float = 0.0, has_time: bool = False) -> np.ndarray:
    """The edge loop of removeObstacle (R/DRRT.jl:3202-3290): edges that start at a node in conflict, are blocked
    (dist == Inf), collide with ob, and with no OTHER obstacle that is in use (the caller's `unused` flags say which
    are; the reference also asks startTime <= timeElapsed <= startTime + lifeSpan, which the caller folds into those
    flags) -- the edges the reference resets to distOriginal.  Ascending edge ids."""
    nodes = set(points_in_conflict_polygon(tree, ps, j, robot_radius, delta, has_time, dubins).tolist())
    out = []
    for e in range(len(e_start)):
        if int(e_start[e]) not in nodes or e_dist[e] != np.inf:
            continue
        a, b = pts[e_start[e]], pts[e_end[e]]
        if not explicit_edge_check_obstacle(ps, j, a, b, robot_radius, dubins, r_min, has_time):
            continue
        other = False
        for k in range(ps.m):
            if k != j and not ps.arr[k].unused and explicit_edge_check_obstacle(ps, k, a, b, robot_radius, dubins, r_min, has_time):
                other = True
                break
        if not other:
            out.append(e)
    return np.array(out, dtype=np.int32)


def dubins_steer(s, g, r_min: float, want_traj: bool = True):
    """Returns (cost, word, traj[P,2])."""
    s, g = _vec(s), _vec(g)
    cost = C.c_double()
    word = C.create_string_buffer(4)
    cap = 1024
    traj = np.zeros((cap, 2), dtype=np.float64)
    n = C.c_int()
    lib().orc_dubins_steer(_dp(s), _dp(g), r_min, C.byref(cost), word, _dp(traj) if want_traj else None,
                           cap, C.byref(n))
    return cost.value, word.value.decode(), traj[: n.value].copy()


def dubins_edge_check_polygons(ps: PolygonSet, s, g, traj, robot_radius, r_min):
    s, g = _vec(s), _vec(g)
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, 2)
    fh = C.c_int32()
    hit = lib().orc_dubins_edge_check_polygons(ps.arr, ps.m, _dp(s), _dp(g), _dp(traj), traj.shape[0],
                                               robot_radius, r_min, C.byref(fh))
    return bool(hit), fh.value


def dubins_steer_time(s, g, r_min: float, piecewise: bool = False):
    """calculateTrajectory(S, ::DubinsEdge) with S.spaceHasTime: (dist, Wdist, velocity, word, traj[P,3]).
    piecewise: the time column as the HIP kernels form it (orc_dubins_steer_time_pw) instead of the reference's
    running sum; the two differ by rounding only."""
    s, g = _vec(s), _vec(g)
    dist, wdist, vel = C.c_double(), C.c_double(), C.c_double()
    word = C.create_string_buffer(4)
    cap = 1024
    traj = np.zeros((cap, 3), dtype=np.float64)
    n = C.c_int()
    fn = lib().orc_dubins_steer_time_pw if piecewise else lib().orc_dubins_steer_time
    fn(_dp(s), _dp(g), r_min, C.byref(dist), C.byref(wdist), C.byref(vel), word, _dp(traj), cap, C.byref(n))
    return dist.value, wdist.value, vel.value, word.value.decode(), traj[: n.value].copy()


DM_SIN, DM_COS, DM_ATAN2, DM_ACOS = 0, 1, 2, 3


def dm_eval(op: int, x, y=None) -> np.ndarray:
    """include/rrtx_detmath.h element-wise on the host: sin(x), cos(x), atan2(y, x), acos(x)."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = x if y is None else np.ascontiguousarray(y, dtype=np.float64).ravel()
    assert x.shape == y.shape
    out = np.empty_like(x)
    rc = lib().orc_dm_eval(op, _dp(x), _dp(y), x.size, _dp(out))
    assert rc == 0, "the default oracle build must not be the libm cross-check build"
    return out


def libm_variant() -> C.CDLL:
    """librrtx_oracle_libm.so: the Dubins functions with glibc's transcendentals (orc_dubins_steer only is bound)."""
    build()
    L = C.CDLL(_LIBM_PATH)
    L.orc_dubins_steer.argtypes = [c_double_p, c_double_p, C.c_double, c_double_p, C.c_char_p,
                                   c_double_p, C.c_int, C.POINTER(C.c_int)]
    L.orc_dm_eval.restype = C.c_int
    L.orc_dm_eval.argtypes = [C.c_int, c_double_p, c_double_p, C.c_int64, c_double_p]
    return L


def dubins_valid_move_time(s, g, velocity: float, v_min: float, v_max: float) -> bool:
    s, g = _vec(s), _vec(g)
    return bool(lib().orc_dubins_valid_move_time(_dp(s), _dp(g), velocity, v_min, v_max))


def dubins_edge_check_polygons_time(ps: "PolygonSet", s, g, traj3, robot_radius, r_min):
    s, g = _vec(s), _vec(g)
    traj3 = np.ascontiguousarray(traj3, dtype=np.float64).reshape(-1, 3)
    fh = C.c_int32()
    hit = lib().orc_dubins_edge_check_polygons_time(ps.arr, ps.m, _dp(s), _dp(g), _dp(traj3), traj3.shape[0],
                                                    robot_radius, r_min, C.byref(fh))
    return bool(hit), fh.value


class Graph:
    """The reference's cost propagation on an index graph (rrtx_oracle_graph.c): rrtLMC / rrtTreeCost per node,
    edges with dist, the rrtXQueue heap and the orphan stack; methods carry the reference's names."""

    def __init__(self, n: int):
        self.n = n
        self._h = C.c_void_p(lib().orc_graph_create(n))

    def __del__(self):
        try:
            lib().orc_graph_destroy(self._h)
        except Exception:
            pass

    def add_edge(self, start: int, end: int, dist: float, initial: bool = False, valid_move: bool = True) -> int:
        return lib().orc_graph_add_edge(self._h, start, end, dist, 1 if initial else 0, 1 if valid_move else 0)

    def add_edges(self, start, end, dist, initial: bool = False, valid_move: bool = True) -> int:
        """add_edge for every start[i] -> end[i] with dist[i], in order, in C; returns the first id"""
        s = np.ascontiguousarray(start, dtype=np.int32).reshape(-1)
        e = np.ascontiguousarray(end, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        assert s.shape == e.shape == w.shape
        assert s.size == 0 or (0 <= min(s.min(), e.min()) and max(s.max(), e.max()) < self.n)
        return lib().orc_graph_add_edges(self._h, _at(s), _at(e), _at(w), s.size, 1 if initial else 0,
                                         1 if valid_move else 0)

    def _read(self, which: str) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int64 if which == "parent_edge" else np.float64)
        args = [None, None, None]
        args[("lmc", "tree_cost", "parent_edge").index(which)] = _at(out)
        lib().orc_graph_read(self._h, *args)
        return out

    def set_node(self, v: int, lmc: float, tree_cost: float):
        lib().orc_graph_set_node(self._h, v, lmc, tree_cost)

    def set_move_goal(self, v: int, flag: bool = True):
        lib().orc_graph_set_move_goal(self._h, v, 1 if flag else 0)

    def set_edge_dist(self, e: int, dist: float):
        lib().orc_graph_set_edge_dist(self._h, e, dist)

    def lmc(self):
        return self._read("lmc")

    def tree_cost(self):
        return self._read("tree_cost")

    def parent_edge(self):
        return self._read("parent_edge")

    def queue_length(self) -> int:
        return lib().orc_graph_queue_length(self._h)

    def verifyInQueue(self, v: int):
        lib().orc_graph_verify_in_queue(self._h, v)

    def verifyInOSQueue(self, v: int):
        lib().orc_graph_verify_in_os(self._h, v)

    def makeParentOf(self, new_parent: int, node: int, edge: int):
        lib().orc_graph_make_parent_of(self._h, new_parent, node, edge)

    def reduceInconsistency(self, goal: int, root: int, hyberBallRad: float = float("inf"), changeThresh: float = 0.0):
        lib().orc_graph_reduce_inconsistency(self._h, goal, root, hyberBallRad, changeThresh)

    def blockEdge(self, e: int):
        """addNewObstacle's handling of one edge the new obstacle hits (R/DRRT_Q.jl:3248-3268)"""
        lib().orc_graph_block_edge(self._h, e)

    def block_edges(self, ids):
        """blockEdge for every id, in the order given, in C"""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        assert ids.size == 0 or (0 <= ids.min() and ids.max() < lib().orc_graph_n_edges(self._h))
        lib().orc_graph_block_edges(self._h, _at(ids), ids.size)

    def propogateDescendants(self):
        lib().orc_graph_propagate_descendants(self._h)


def julia_range_len(start, step, stop) -> int:
    return lib().orc_julia_range_len(start, step, stop)


def extend_batch_polygons(tree: KDTree, ps: "PolygonSet", queries: np.ndarray, r: float, robot_radius: float):
    """CPU-baseline loop against a polygon list. Returns (edges_checked, neighbours, hits, nearest_idx)."""
    q = np.ascontiguousarray(queries, dtype=np.float64)
    nq = q.shape[0]
    nearest = np.empty(nq, dtype=np.int64)
    nn, nh = C.c_int64(), C.c_int64()
    e = lib().orc_extend_batch_polygons(tree.handle, ps.arr, ps.m, _dp(q), nq, r, robot_radius,
                                        nearest.ctypes.data_as(c_int64_p), C.byref(nn), C.byref(nh))
    return e, nn.value, nh.value, nearest


def extend_batch_spheres(tree: KDTree, spheres, m, queries: np.ndarray, r: float, robot_radius: float):
    """CPU-baseline loop. Returns (edges_checked, neighbours, hits, nearest_idx)."""
    q = np.ascontiguousarray(queries, dtype=np.float64)
    nq = q.shape[0]
    nearest = np.empty(nq, dtype=np.int64)
    nn, nh = C.c_int64(), C.c_int64()
    e = lib().orc_extend_batch_spheres(tree.handle, spheres, m, _dp(q), nq, r, robot_radius,
                                       nearest.ctypes.data_as(c_int64_p), C.byref(nn), C.byref(nh))
    return e, nn.value, nh.value, nearest


# ---- batched Dubins edges (orc_dubins_edges_batch / orc_dubins_candidates_batch) ----------------------------------
MAX_THREADS = 16


def _n_threads(threads) -> int:
    if threads is None:
        try:
            threads = len(os.sched_getaffinity(0))
        except AttributeError:
            threads = 1
    return max(1, min(MAX_THREADS, int(threads)))


def _at(a, i: int = 0, row: int = 1):
    """address of element i * row of a C-contiguous array (None for None)"""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data + i * row * a.itemsize


def _run_ranges(n: int, threads, fn, per_thread: int = 1024, worker: bool = False):
    """fn(i0, i1) over [0, n) split into contiguous ranges of at least per_thread items, on up to MAX_THREADS threads
    (ctypes drops the GIL); worker=True calls fn(j, i0, i1) with the range's number j < _n_threads(threads)"""
    k = min(_n_threads(threads), max(1, n // per_thread))
    bounds = [n * j // k for j in range(k + 1)]
    call = (lambda j: fn(j, bounds[j], bounds[j + 1])) if worker else (lambda j: fn(bounds[j], bounds[j + 1]))
    if k == 1:
        rcs = [call(0)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(k) as ex:
            rcs = list(ex.map(call, range(k)))
    for rc in rcs:
        if rc == -1:
            raise ValueError("the oracle has no Dubins check without time for a list with active moving obstacles")
        if rc != 0:
            raise RuntimeError(f"oracle Dubins batch failed ({rc})")


def _poly_args(ps):
    return (ps.arr, ps.m) if ps is not None else ((Polygon * 1)(), 0)


def dubins_edges_batch(S, G, r_min: float, ps: "PolygonSet" = None, robot_radius: float = 0.0, has_time: bool = False,
                       piecewise: bool = False, v_min: float = 0.0, v_max: float = 0.0, traj=None, threads=None) -> dict:
    """Every directed edge S[i] -> G[i] through the per-edge Dubins functions (dubins_steer / dubins_steer_time,
    dubins_edge_check_polygons[_time], dubins_valid_move_time), in C.  Returns dict(cost, wdist, velocity, word
    (S3), traj_len, hit, first_hit, valid_move); without ps the check is skipped (hit 0).  traj: True or a boolean
    mask -- also traj_off (n + 1, rows) and traj (rows of 2, or 3 with time) for those edges (zero rows for the
    others)."""
    S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1, 4)
    G = np.ascontiguousarray(G, dtype=np.float64).reshape(-1, 4)
    assert S.shape == G.shape
    n = S.shape[0]
    arr, m = _poly_args(ps)
    L = lib()
    out = dict(cost=np.empty(n), wdist=np.empty(n), velocity=np.empty(n), word=np.zeros((n, 3), dtype=np.uint8),
               traj_len=np.empty(n, dtype=np.int32), hit=np.zeros(n, dtype=np.uint8),
               first_hit=np.full(n, -1, dtype=np.int32), valid_move=np.empty(n, dtype=np.uint8))
    chk = ps is not None

    def run(i0, i1, off=None, rows=None):
        return L.orc_dubins_edges_batch(
            _at(S, i0, 4), _at(G, i0, 4), i1 - i0, r_min, robot_radius, arr, m, int(has_time), int(piecewise), v_min,
            v_max, _at(out["cost"], i0), _at(out["wdist"], i0), _at(out["velocity"], i0), _at(out["word"], i0, 3),
            _at(out["traj_len"], i0), _at(out["hit"], i0) if chk else None, _at(out["first_hit"], i0) if chk else None,
            _at(out["valid_move"], i0), _at(off, i0), _at(rows))
    _run_ranges(n, threads, run)
    out["word"] = out["word"].view("S3").ravel()
    if traj is not None and traj is not False:
        mask = np.ones(n, dtype=bool) if traj is True else np.asarray(traj, dtype=bool).reshape(n)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.where(mask, out["traj_len"], 0), out=off[1:])
        rows = np.zeros((max(int(off[-1]), 1), 3 if has_time else 2))
        arr0, m0 = _poly_args(None)
        _run_ranges(n, threads, lambda i0, i1: L.orc_dubins_edges_batch(
            _at(S, i0, 4), _at(G, i0, 4), i1 - i0, r_min, robot_radius, arr0, m0, int(has_time), int(piecewise), v_min,
            v_max, None, None, None, None, None, None, None, None, _at(off, i0), _at(rows)))
        out["traj_off"], out["traj"] = off, rows[: int(off[-1])]
    return out


def dubins_candidates_batch(Q, offsets, idx, nodes, r_min: float, ps: "PolygonSet", robot_radius: float,
                            has_time: bool = False, piecewise: bool = False, v_min: float = 0.0, v_max: float = 0.0,
                            threads=None) -> dict:
    """The candidate Dubins edges of extend() for CSR entries (sample of the offsets range, node idx[e]), both
    directions, in C: dict(cost_out, cost_in, hit_out, hit_in, traj_len_out, traj_len_in); the hit bytes are
    rrtx_extend_candidates_dubins's flags (bit 0 collision, bit 1 invalid move with time)."""
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 4)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 4)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    nq = Q.shape[0]
    assert offsets.shape == (nq + 1,) and int(offsets[-1]) == idx.shape[0]
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < nodes.shape[0])
    n = idx.shape[0]
    arr, m = ps.arr, ps.m
    L = lib()
    out = dict(cost_out=np.empty(n), cost_in=np.empty(n), hit_out=np.empty(n, dtype=np.uint8),
               hit_in=np.empty(n, dtype=np.uint8), traj_len_out=np.empty(n, dtype=np.int32),
               traj_len_in=np.empty(n, dtype=np.int32))
    _run_ranges(n, threads, lambda e0, e1: L.orc_dubins_candidates_batch(
        _at(Q), nq, _at(offsets), _at(idx), _at(nodes), e0, e1, r_min, robot_radius, arr, m, int(has_time),
        int(piecewise), v_min, v_max, _at(out["cost_out"]), _at(out["cost_in"]), _at(out["hit_out"]),
        _at(out["hit_in"]), _at(out["traj_len_out"]), _at(out["traj_len_in"])))
    return out


# ---- batched search and SimpleEdge checks (orc_range_batch, orc_knearest_batch, orc_simple_candidates_batch,
#      orc_edges_check_batch, orc_points_check_batch) ------------------------------------------------------------------
RANGE_SLICE = 64           # samples per orc_range_batch call: a capacity retry repeats one slice, not a thread's range


class TreeSet:
    """One KDTree per worker thread over the same points, built in insertion order: the range and k-nearest
    searches mark the nodes they visit in the tree, so two threads never search one tree."""

    def __init__(self, d: int, pts=None, threads=None, wraps=None, wrap_points=None):
        self.d = d
        self.trees = [KDTree(d, wraps, wrap_points) for _ in range(_n_threads(threads))]
        if pts is not None:
            self.insert_many(pts)

    def insert_many(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, self.d)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(len(self.trees)) as ex:
            list(ex.map(lambda t: t.insert_many(pts), self.trees))

    @property
    def size(self) -> int:
        return self.trees[0].size


def _tree_list(trees):
    return trees.trees if isinstance(trees, TreeSet) else [trees]


def range_batch(trees, Q, r, per_sample: float = 64.0, nearest: bool = True, slice_size: int = RANGE_SLICE) -> dict:
    """kdFindWithinRange (r: scalar or one radius per sample) and kdFindNearest for every sample, in C, on the trees
    of a TreeSet (one per thread) or on one KDTree: dict(offsets, idx, key, nearest_idx, nearest_dist, retries) --
    CSR with each list in ascending node index, as the device returns it.  per_sample seeds each slice's capacity
    (a device count may seed it; the result never depends on it): a slice that needs more is searched again with
    the size it needs, counted in retries."""
    ts = _tree_list(trees)
    d = ts[0].d
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, d)
    nq = Q.shape[0]
    rr = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    stride = 0 if rr.size == 1 else 1
    if stride and rr.size != nq:
        raise ValueError("r must be a scalar or have one entry per sample")
    nidx = np.empty(nq, dtype=np.int64)
    ndist = np.empty(nq, dtype=np.float64)
    n_slices = (nq + slice_size - 1) // slice_size
    parts = [None] * n_slices
    retries = [0] * len(ts)
    L = lib()

    def run(j, s0, s1):
        t = ts[j].handle
        for s in range(s0, s1):
            a = s * slice_size
            n = min(nq, a + slice_size) - a
            cap = int(per_sample * n) + 64
            while True:
                off = np.empty(n + 1, dtype=np.int64)
                idx = np.empty(cap, dtype=np.int32)
                key = np.empty(cap, dtype=np.float64)
                need = L.orc_range_batch(t, _at(Q, a, d), n, _at(rr, a * stride), stride, cap, _at(off), _at(idx),
                                         _at(key), _at(nidx, a) if nearest else None, _at(ndist, a) if nearest else None)
                if need < 0:
                    raise MemoryError("orc_range_batch")
                if need <= cap:
                    break
                cap = int(need)
                retries[j] += 1
            parts[s] = (np.diff(off), idx[:need], key[:need])
        return 0
    _run_ranges(n_slices, len(ts), run, per_thread=1, worker=True)
    offsets = np.zeros(nq + 1, dtype=np.int64)
    if n_slices:
        np.cumsum(np.concatenate([p[0] for p in parts]), out=offsets[1:])
    out = dict(offsets=offsets,
               idx=np.concatenate([p[1] for p in parts]) if n_slices else np.empty(0, dtype=np.int32),
               key=np.concatenate([p[2] for p in parts]) if n_slices else np.empty(0), retries=sum(retries))
    if nearest:
        out["nearest_idx"], out["nearest_dist"] = nidx, ndist
    return out


def knearest_batch(trees, k: int, Q) -> tuple:
    """kdFindKNearest for every sample, in C: (idx, key, count), rows max(k, 2) wide in heap order, count[i] of row i
    filled; raises where the reference does (wrapped space)."""
    ts = _tree_list(trees)
    d = ts[0].d
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, d)
    nq = Q.shape[0]
    w = max(int(k), 2)
    idx = np.full((nq, w), -1, dtype=np.int32)
    key = np.full((nq, w), np.nan)
    count = np.empty(nq, dtype=np.int32)
    L = lib()

    def run(j, i0, i1):
        rc = L.orc_knearest_batch(ts[j].handle, int(k), _at(Q, i0, d), i1 - i0, w, _at(idx, i0, w), _at(key, i0, w),
                                  _at(count, i0))
        if rc == -1:
            raise RuntimeError("knn search has not been implimented for wrapped space")
        return rc
    _run_ranges(nq, len(ts), run, per_thread=64, worker=True)
    return idx, key, count


def _obs_args(obs):
    """(spheres, polygons, m) for the batch functions: obs is a PolygonSet or make_spheres()'s (array, m)"""
    if isinstance(obs, PolygonSet):
        return None, C.addressof(obs.arr), obs.m
    arr, m = obs
    return C.addressof(arr), None, m


def candidates_batch(Q, offsets, idx, nodes, obs, robot_radius: float, threads=None) -> dict:
    """The SimpleEdge candidate edges of extend() for CSR entries (sample of the offsets range, node idx[e]), both
    directions, in C: dict(cost_out, cost_in, hit_out, hit_in, first_hit_out, first_hit_in)."""
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    d = nodes.shape[1]
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, d)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    nq = Q.shape[0]
    assert offsets.shape == (nq + 1,) and int(offsets[-1]) == idx.shape[0]
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < nodes.shape[0])
    n = idx.shape[0]
    sph, poly, m = _obs_args(obs)
    out = dict(cost_out=np.empty(n), cost_in=np.empty(n), hit_out=np.empty(n, dtype=np.uint8),
               hit_in=np.empty(n, dtype=np.uint8), first_hit_out=np.empty(n, dtype=np.int32),
               first_hit_in=np.empty(n, dtype=np.int32))
    L = lib()

    def run(e0, e1):
        return L.orc_simple_candidates_batch(_at(Q), nq, d, _at(offsets), _at(idx), _at(nodes), e0, e1, sph, poly, m,
                                             robot_radius, *(_at(out[k]) for k in ("cost_out", "cost_in", "hit_out",
                                                                                    "hit_in", "first_hit_out",
                                                                                    "first_hit_in")))
    if n:
        _run_ranges(n, threads, run)
    return out


def edges_check_batch(obs, P0, P1, robot_radius: float, threads=None):
    """explicitEdgeCheck over the list for every directed edge P0[i] -> P1[i], in C: (hit, first_hit)"""
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    assert P0.shape == P1.shape and P0.ndim == 2
    n, d = P0.shape
    sph, poly, m = _obs_args(obs)
    hit = np.empty(n, dtype=np.uint8)
    first = np.empty(n, dtype=np.int32)
    L = lib()
    _run_ranges(n, threads, lambda i0, i1: L.orc_edges_check_batch(_at(P0, i0, d), _at(P1, i0, d), i1 - i0, d, sph,
                                                                   poly, m, robot_radius, _at(hit, i0),
                                                                   _at(first, i0)) or 0)
    return hit, first


def points_check_batch(obs, P, robot_radius: float, quick: bool = True, threads=None):
    """explicitPointCheck over the list for every point, in C (quick pass first for spheres): (unsafe, clearance)"""
    P = np.ascontiguousarray(P, dtype=np.float64)
    n, d = P.shape
    sph, poly, m = _obs_args(obs)
    unsafe = np.empty(n, dtype=np.uint8)
    clr = np.empty(n, dtype=np.float64)
    L = lib()
    _run_ranges(n, threads, lambda i0, i1: L.orc_points_check_batch(_at(P, i0, d), i1 - i0, d, sph, poly, m,
                                                                    robot_radius, int(quick), _at(unsafe, i0),
                                                                    _at(clr, i0)) or 0)
    return unsafe, clr


EDGE_SIMPLE, EDGE_DUBINS, EDGE_DUBINS_TIME = 0, 1, 2


def sweep_edges_batch(nodes, es, ee, in_conflict, obs, j: int, robot_radius: float, edge: int = EDGE_SIMPLE,
                      remove: bool = False, dist=None, r_min: float = 0.0, threads=None) -> np.ndarray:
    """The edge loop of addNewObstacle (remove: removeObstacle) over the mirror es -> ee, in C: the ids (ascending, as
    add_new_obstacle_edges / remove_obstacle_edges return them) of the edges that start at a node with
    in_conflict[node] set and for which explicitEdgeCheck(S, edge, obs[j]) is true; remove: that also have
    dist == Inf and hit no other obstacle of the list in use.  obs is a PolygonSet or make_spheres()'s (array, m)
    (SimpleEdge only); edge is EDGE_SIMPLE, EDGE_DUBINS or EDGE_DUBINS_TIME (the piecewise time column)."""
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    d = nodes.shape[1]
    es = np.ascontiguousarray(es, dtype=np.int32).reshape(-1)
    ee = np.ascontiguousarray(ee, dtype=np.int32).reshape(-1)
    mask = np.ascontiguousarray(in_conflict, dtype=np.uint8).reshape(-1)
    assert es.shape == ee.shape and mask.shape == (nodes.shape[0],)
    assert es.size == 0 or (0 <= min(es.min(), ee.min()) and max(es.max(), ee.max()) < nodes.shape[0])
    w = None
    if remove:
        w = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        assert w.shape == es.shape
    sph, poly, m = _obs_args(obs)
    if not 0 <= j < m:
        raise IndexError(f"obstacle {j} of a list of {m}")
    sel = np.zeros(es.size, dtype=np.uint8)
    L = lib()
    _run_ranges(es.size, threads, lambda e0, e1: L.orc_sweep_edges_batch(
        _at(es), _at(ee), _at(w), e0, e1, _at(nodes), d, _at(mask), sph, poly, m, int(j), int(remove), int(edge),
        robot_radius, r_min, _at(sel)), per_thread=4096)
    return np.flatnonzero(sel).astype(np.int32)


def extend_candidates_batch(trees, Q, r: float, nodes, obs, robot_radius: float, rng: dict = None,
                            per_sample: float = 64.0, threads=None) -> dict:
    """What rrtx_extend_candidates returns, from the oracle: range_batch (or a given result of it for the same
    samples, radius and tree), the candidate edges of every entry and the sample check.  Keys of the device call
    (offsets, idx, cost, hit_out, hit_in, nearest_idx, nearest_dist, sample_unsafe) plus key, cost_in,
    first_hit_out, first_hit_in."""
    if rng is None:
        rng = range_batch(trees, Q, r, per_sample=per_sample)
    c = candidates_batch(Q, rng["offsets"], rng["idx"], nodes, obs, robot_radius, threads=threads)
    unsafe, _ = points_check_batch(obs, np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, nodes.shape[1]),
                                   robot_radius, quick=True, threads=threads)
    return dict(offsets=rng["offsets"], idx=rng["idx"], cost=c["cost_out"], hit_out=c["hit_out"], hit_in=c["hit_in"],
                nearest_idx=rng["nearest_idx"], nearest_dist=rng["nearest_dist"], sample_unsafe=unsafe,
                key=rng["key"], cost_in=c["cost_in"], first_hit_out=c["first_hit_out"],
                first_hit_in=c["first_hit_in"])


# ---- comparing device results with these, naming the first difference -----------------------------------------------
ENTRY_FIELDS = ("idx", "key", "cost", "cost_in", "hit_out", "hit_in", "first_hit_out", "first_hit_in")
SAMPLE_FIELDS = ("nearest_idx", "nearest_dist", "sample_unsafe")


def take_samples(res: dict, sel) -> dict:
    """The rows sel of a CSR result (offsets + ENTRY_FIELDS + SAMPLE_FIELDS that it has), as a CSR of its own"""
    off = np.asarray(res["offsets"], dtype=np.int64)
    sel = np.asarray(sel, dtype=np.int64)
    counts = off[sel + 1] - off[sel]
    new_off = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(counts, out=new_off[1:])
    ent = np.repeat(off[sel], counts) + (np.arange(int(new_off[-1])) - np.repeat(new_off[:-1], counts))
    out = {"offsets": new_off}
    for k, v in res.items():
        if k in ENTRY_FIELDS:
            out[k] = np.asarray(v)[ent]
        elif k in SAMPLE_FIELDS:
            out[k] = np.asarray(v)[sel]
    return out


def _bits_equal(a, b) -> np.ndarray:
    """element-wise: equal values with equal signs (0.0 vs -0.0 differ), or both NaN"""
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = a.astype(np.float64), b.astype(np.float64)
        return ((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))
    return a == b


def assert_same_results(dev: dict, ref: dict, fields, names=None, label: str = ""):
    """dev == ref bit for bit in every field named (offsets, ENTRY_FIELDS, SAMPLE_FIELDS) of the CSR; on a
    difference, raise naming the first differing sample (names[i] for row i, default i), the field and both values."""
    off = np.asarray(ref["offsets"], dtype=np.int64)
    n = len(off) - 1
    names = np.arange(n) if names is None else np.asarray(names)
    if "offsets" in fields:
        od = np.asarray(dev["offsets"], dtype=np.int64)
        if od.shape != off.shape:
            raise AssertionError(f"{label}offsets: {len(od) - 1} samples on the device, {n} in the oracle")
        cd, cr = np.diff(od), np.diff(off)
        bad = np.flatnonzero(cd != cr)
        if bad.size:
            i = int(bad[0])
            a = np.asarray(dev["idx"])[od[i]:od[i + 1]] if "idx" in dev else np.zeros(0)
            b = np.asarray(ref["idx"])[off[i]:off[i + 1]] if "idx" in ref else np.zeros(0)
            k = min(len(a), len(b))
            j = int(np.flatnonzero(a[:k] != b[:k])[0]) if (a[:k] != b[:k]).any() else k
            da = int(a[j]) if j < len(a) else None
            db = int(b[j]) if j < len(b) else None
            raise AssertionError(f"{label}sample {names[i]}: field idx: {cd[i]} neighbours on the device, {cr[i]} in the "
                                 f"oracle; first difference at entry {j}: device node {da}, oracle node {db}")
        if not np.array_equal(od, off):
            raise AssertionError(f"{label}offsets: device offsets do not start at 0")
    for k in fields:
        if k == "offsets":
            continue
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        if a.shape != b.shape:
            raise AssertionError(f"{label}field {k}: shape {a.shape} on the device, {b.shape} in the oracle")
        ok = _bits_equal(a, b)
        if ok.all():
            continue
        e = np.unravel_index(int(np.flatnonzero(~ok.ravel())[0]), a.shape)
        if k in SAMPLE_FIELDS or k not in ENTRY_FIELDS:
            where = f"sample {names[e[0]]}" + (f" column {e[1]}" if len(e) > 1 else "")
        else:
            s = int(np.searchsorted(off, e[0], side="right") - 1)
            where = f"sample {names[s]} entry {e[0] - off[s]} (node {np.asarray(ref['idx'])[e[0]] if 'idx' in ref else '?'})"
        raise AssertionError(f"{label}{where}: field {k}: device {a[e]!r}, oracle {b[e]!r} "
                             f"({int((~ok).sum())} of {ok.size} differ)")
