"""numpy-facing wrapper of one rrtx_ctx (one tree + obstacle lists on one GPU).

Thin by design: every method is one C-ABI call of include/rrtx.h.  The
reference-named API (kdInsert, kdFindWithinRange, explicitEdgeCheck, ...) lives in
rrtqx_3d_amd/drrt.py on top of this.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import RrtxError, Stats, f64


class Context:
    def __init__(self, dim: int = 3, device: int = 0, node_capacity: int = 1024):
        self._lib = _capi.load()
        _capi.verify_runtime()      # one HIP runtime image per process, or refuse
        self.dim = dim
        self.device = device
        h = C.c_void_p()
        rc = self._lib.rrtx_create(C.byref(h), dim, device, node_capacity)
        if rc != _capi.RRTX_OK:
            raise RrtxError(rc, self._lib.rrtx_create_error().decode())
        self._h = h
        self._registered = []       # arrays this object page-locked (select_out_buffers): alive until close()

    # ---- lifetime -------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for a in getattr(self, "_registered", []):
                self._lib.rrtx_host_unregister(self._h, a.ctypes.data)
            self._registered = []
            self._lib.rrtx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != _capi.RRTX_OK:
            raise RrtxError(rc, self._lib.rrtx_last_error(self._h).decode())

    def _two_call(self, cap: int, call):
        """The two-call pattern: call(cap, needed) allocates room for cap entries and makes the C call with `needed`
        as its count output, returning (rc, arrays); RRTX_E_CAPACITY repeats it with cap = needed.
        Returns (needed, arrays)."""
        while True:
            needed = C.c_int64()
            rc, arrays = call(cap, C.byref(needed))
            if rc != _capi.RRTX_E_CAPACITY:
                self._check(rc)
                return int(needed.value), arrays
            cap = int(needed.value)

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: Optional[int]):
        self._check(self._lib.rrtx_set_stream(self._h, stream_ptr))

    def get_stream(self) -> int:
        return self._lib.rrtx_get_stream(self._h) or 0

    def sync(self):
        self._check(self._lib.rrtx_sync(self._h))

    def profile(self, level):
        """0/False off, 1 range-scan kernel only, 2/True every kernel family."""
        lvl = 2 if level is True else int(level)
        self._check(self._lib.rrtx_profile(self._h, lvl))

    def set_option(self, option: int, value: int):
        self._check(self._lib.rrtx_set_option(self._h, option, value))

    def get_option(self, option: int) -> int:
        v = C.c_int64()
        self._check(self._lib.rrtx_get_option(self._h, option, C.byref(v)))
        return int(v.value)

    def last_tile_form(self) -> int:
        """rrtx_last_tile_form: 0 no tile kernel in the last range search, 1 its looped form, 2 its straight form"""
        v = C.c_int()
        self._check(self._lib.rrtx_last_tile_form(self._h, C.byref(v)))
        return int(v.value)

    @property
    def space_has_time(self) -> bool:
        """CSpace.spaceHasTime as the CONTEXT holds it (no shadow copy: buffers are sized from this)."""
        return self.get_option(_capi.RRTX_OPT_SPACE_HAS_TIME) != 0

    @property
    def dubins_time_column(self) -> int:
        """RRTX_OPT_DUBINS_TIME_COLUMN as the context holds it: _capi.RRTX_TIME_COLUMN_PIECEWISE or _RUNNING_SUM."""
        return self.get_option(_capi.RRTX_OPT_DUBINS_TIME_COLUMN)

    def stats(self) -> Stats:
        s = Stats()
        self._check(self._lib.rrtx_stats(self._h, C.byref(s)))
        return s

    # ---- tree -------------------------------------------------------------------
    def nodes_append(self, pos) -> int:
        pos = f64(pos, (-1, self.dim))
        first = C.c_int64()
        self._check(self._lib.rrtx_nodes_append(self._h, _capi._ptr(pos), pos.shape[0], C.byref(first)))
        return first.value

    def nodes_append_dev(self, dev_ptr: int, n: int):
        self._check(self._lib.rrtx_nodes_append_dev(self._h, dev_ptr, n))

    @property
    def n_nodes(self) -> int:
        return self._lib.rrtx_nodes_count(self._h)

    def set_wrap(self, dim_index: int, period: float):
        self._check(self._lib.rrtx_set_wrap(self._h, dim_index, period))

    # ---- obstacles ----------------------------------------------------------------
    def spheres_set(self, cxyzr, active=None):
        cxyzr = f64(cxyzr, (-1, 4))
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        self._check(self._lib.rrtx_spheres_set(self._h, _capi._ptr(cxyzr), _capi._ptr(act), cxyzr.shape[0]))

    def obstacle_update(self, which: int, radius: float, active: bool):
        self._check(self._lib.rrtx_obstacle_update(self._h, which, radius, 1 if active else 0))

    def polygons_set(self, polys, kinds=None, active=None, centre_radius=None, paths=None):
        """polys: list of (P_i x 2) vertex arrays in list order; paths: per obstacle an (M_i x 3) array of
        (dx, dy, t) rows for the moving kinds 6 / 7 (None or empty for the others)."""
        polys = [f64(p, (-1, 2)) for p in polys]
        m = len(polys)
        off = np.zeros(m + 1, dtype=np.int32)
        for i, p in enumerate(polys):
            off[i + 1] = off[i] + p.shape[0]
        vxy = np.concatenate(polys, axis=0) if m else np.zeros((0, 2))
        vxy = f64(vxy, (-1, 2))
        k = None if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8)
        a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        cr = None if centre_radius is None else f64(centre_radius, (-1, 3))
        self._check(self._lib.rrtx_polygons_set(self._h, _capi._ptr(off), _capi._ptr(vxy), _capi._ptr(cr),
                                                _capi._ptr(k), _capi._ptr(a), m))
        if paths is not None:
            self.polygon_paths_set(paths)

    def polygon_paths_set(self, paths):
        """Obstacle.path of every polygon obstacle (list order); see rrtx_polygon_paths_set."""
        rows = [np.zeros((0, 3)) if p is None else f64(p, (-1, 3)) for p in paths]
        m = len(rows)
        off = np.zeros(m + 1, dtype=np.int32)
        for i, p in enumerate(rows):
            off[i + 1] = off[i] + p.shape[0]
        xyt = f64(np.concatenate(rows, axis=0) if m else np.zeros((0, 3)), (-1, 3))
        self._check(self._lib.rrtx_polygon_paths_set(self._h, _capi._ptr(off), _capi._ptr(xyt), m))

    # ---- nearest neighbours ---------------------------------------------------------
    def nn_nearest(self, q) -> Tuple[np.ndarray, np.ndarray]:
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        idx = np.empty(nq, dtype=np.int32)
        dist = np.empty(nq, dtype=np.float64)
        self._check(self._lib.rrtx_nn_nearest(self._h, _capi._ptr(q), nq, _capi._ptr(idx), _capi._ptr(dist)))
        return idx, dist

    def nn_knearest(self, q, k: int):
        """kdFindKNearest per query: (idx, dist, count); rows are max(k, 2) wide, sorted by
        (distance, index), count[i] entries of row i are filled."""
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        stride = max(int(k), 2)
        idx = np.empty((nq, stride), dtype=np.int32)
        dist = np.empty((nq, stride), dtype=np.float64)
        count = np.empty(nq, dtype=np.int32)
        self._check(self._lib.rrtx_nn_knearest(self._h, _capi._ptr(q), nq, int(k), _capi._ptr(idx), _capi._ptr(dist),
                                               _capi._ptr(count)))
        return idx, dist, count

    def nn_radius(self, q, r, cap: Optional[int] = None):
        """Returns CSR (offsets[nq+1], idx, dist). r: scalar or per-query array."""
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        r_arr = f64(r, (-1,))
        stride = 0 if r_arr.shape[0] == 1 else 1
        if stride == 1 and r_arr.shape[0] != nq:
            raise ValueError("r must be a scalar or have one entry per query")
        if cap is None:
            cap = max(64 * nq, 1024)
        offsets = np.empty(nq + 1, dtype=np.int64)

        def call(cap, needed):
            idx = np.empty(cap, dtype=np.int32)
            dist = np.empty(cap, dtype=np.float64)
            return self._lib.rrtx_nn_radius(self._h, _capi._ptr(q), _capi._ptr(r_arr), stride, nq, _capi._ptr(offsets),
                                            _capi._ptr(idx), _capi._ptr(dist), cap, needed), (idx, dist)
        n, (idx, dist) = self._two_call(cap, call)
        return offsets, idx[:n], dist[:n]

    # ---- collision ---------------------------------------------------------------------
    def edges_check(self, p0, p1, robot_radius: float, kind: int = 0, obstacle: int = -1,
                    want_first: bool = True):
        p0 = f64(p0, (-1, self.dim))
        p1 = f64(p1, (-1, self.dim))
        ne = p0.shape[0]
        hit = np.empty(ne, dtype=np.uint8)
        first = np.empty(ne, dtype=np.int32) if want_first else None
        self._check(self._lib.rrtx_edges_check(self._h, kind, _capi._ptr(p0), _capi._ptr(p1), ne, robot_radius,
                                               obstacle, _capi._ptr(hit), _capi._ptr(first)))
        return hit, first

    def points_check(self, p, robot_radius: float, kind: int = 0, quick: bool = True, want_clearance: bool = True):
        p = f64(p, (-1, self.dim))
        n = p.shape[0]
        unsafe = np.empty(n, dtype=np.uint8)
        clr = np.empty(n, dtype=np.float64) if want_clearance else None
        self._check(self._lib.rrtx_points_check(self._h, kind, _capi._ptr(p), n, robot_radius, 1 if quick else 0,
                                                _capi._ptr(unsafe), _capi._ptr(clr) if want_clearance else None))
        return unsafe, clr

    # ---- steering -------------------------------------------------------------------------
    def simple_steer(self, s, g):
        s = f64(s, (-1, self.dim))
        g = f64(g, (-1, self.dim))
        ne = s.shape[0]
        dist = np.empty(ne, dtype=np.float64)
        wdist = np.empty(ne, dtype=np.float64)
        self._check(self._lib.rrtx_simple_steer(self._h, _capi._ptr(s), _capi._ptr(g), ne, _capi._ptr(dist),
                                                _capi._ptr(wdist)))
        return dist, wdist

    def dubins_steer(self, s, g, r_min: float):
        s = f64(s, (-1, 4))
        g = f64(g, (-1, 4))
        ne = s.shape[0]
        cost = np.empty(ne, dtype=np.float64)
        word = np.empty((ne, 3), dtype=np.uint8)
        self._check(self._lib.rrtx_dubins_steer(self._h, _capi._ptr(s), _capi._ptr(g), ne, r_min, _capi._ptr(cost),
                                                _capi._ptr(word)))
        return cost, word.view("S3").ravel()      # numpy bytes array: b"rsl", b"rsr", ...

    def set_space_has_time(self, has_time: bool):
        """CSpace.spaceHasTime for the Dubins entry points (dim = 4: [x y t theta])."""
        self.set_option(_capi.RRTX_OPT_SPACE_HAS_TIME, 1 if has_time else 0)

    def set_dubins_time_column(self, value: int):
        """How the time column of a Dubins edge's polyline is formed in a space with time: RRTX_TIME_COLUMN_PIECEWISE
        (default) or RRTX_TIME_COLUMN_RUNNING_SUM, the reference's own sum (include/rrtx.h); anything else raises."""
        self.set_option(_capi.RRTX_OPT_DUBINS_TIME_COLUMN, int(value))

    def set_dubins_velocity(self, v_min: float, v_max: float):
        """S.dubinsMinVelocity / S.dubinsMaxVelocity (validMove in a space with time)."""
        self._check(self._lib.rrtx_set_dubins_velocity(self._h, float(v_min), float(v_max)))

    def dubins_steer_full(self, s, g, r_min: float):
        """calculateTrajectory's scalars: dict(dist, wdist, velocity, word, valid_move)."""
        s = f64(s, (-1, 4))
        g = f64(g, (-1, 4))
        ne = s.shape[0]
        dist = np.empty(ne, dtype=np.float64)
        wdist = np.empty(ne, dtype=np.float64)
        vel = np.empty(ne, dtype=np.float64)
        word = np.empty((ne, 3), dtype=np.uint8)
        valid = np.empty(ne, dtype=np.uint8)
        self._check(self._lib.rrtx_dubins_steer_full(self._h, _capi._ptr(s), _capi._ptr(g), ne, r_min, _capi._ptr(dist),
                                                     _capi._ptr(wdist), _capi._ptr(vel), _capi._ptr(word),
                                                     _capi._ptr(valid)))
        return dict(dist=dist, wdist=wdist, velocity=vel, word=word.view("S3").ravel(), valid_move=valid)

    def dubins_edges_check(self, s, g, r_min: float, robot_radius: float):
        s = f64(s, (-1, 4))
        g = f64(g, (-1, 4))
        ne = s.shape[0]
        cost = np.empty(ne, dtype=np.float64)
        word = np.empty((ne, 3), dtype=np.uint8)
        hit = np.empty(ne, dtype=np.uint8)
        tl = np.empty(ne, dtype=np.int32)
        self._check(self._lib.rrtx_dubins_edges_check(self._h, _capi._ptr(s), _capi._ptr(g), ne, r_min,
                                                      robot_radius, _capi._ptr(cost), _capi._ptr(word),
                                                      _capi._ptr(hit), _capi._ptr(tl)))
        return cost, word.view("S3").ravel(), hit, tl

    def dubins_trajectory(self, s, g, r_min: float):
        """edge.trajectory of every Dubins edge: (traj_off[ne+1] in rows, traj[rows, 2]) -- rows of
        (x, y, t) in a space with time (set_space_has_time)."""
        s = f64(s, (-1, 4))
        g = f64(g, (-1, 4))
        ne = s.shape[0]
        off = np.empty(ne + 1, dtype=np.int64)
        cap = max(64 * ne, 64)
        cols = 3 if self.space_has_time else 2

        def call(cap, needed):
            xy = np.empty((cap, cols), dtype=np.float64)
            return self._lib.rrtx_dubins_trajectory(self._h, _capi._ptr(s), _capi._ptr(g), ne, r_min, _capi._ptr(off),
                                                    _capi._ptr(xy), cols, cap, needed), xy
        n, xy = self._two_call(cap, call)
        return off, xy[:n]

    def detmath_eval(self, op: int, x, y=None):
        """include/rrtx_detmath.h on the device, element-wise: 0 sin(x), 1 cos(x), 2 atan2(y, x), 3 acos(x)."""
        x = f64(x, (-1,))
        y = x if y is None else f64(y, (-1,))
        out = np.empty_like(x)
        self._check(self._lib.rrtx_detmath_eval(self._h, op, _capi._ptr(x), _capi._ptr(y), x.size, _capi._ptr(out)))
        return out

    # ---- fused extend() preamble --------------------------------------------------------------
    def host_register(self, arr: np.ndarray):
        """Page-lock a caller array that outlives many calls (rrtx_host_register): output pointers inside it receive
        their results by direct DMA instead of through the context's staging arena."""
        assert arr.flags["C_CONTIGUOUS"]
        self._check(self._lib.rrtx_host_register(self._h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr: np.ndarray):
        self._check(self._lib.rrtx_host_unregister(self._h, arr.ctypes.data))

    def extend_out_buffers(self, nq: int, cap: int, register: bool = False) -> dict:
        """Output arrays for extend_candidates(..., out=...) that a caller keeps across calls, as a Julia host does
        (one allocation; register=True page-locks them)."""
        out = dict(offsets=np.empty(nq + 1, dtype=np.int64), idx=np.empty(cap, dtype=np.int32),
                   cost=np.empty(cap, dtype=np.float64), hit_out=np.empty(cap, dtype=np.uint8),
                   hit_in=np.empty(cap, dtype=np.uint8), nearest_idx=np.empty(nq, dtype=np.int32),
                   nearest_dist=np.empty(nq, dtype=np.float64), sample_unsafe=np.empty(nq, dtype=np.uint8))
        if register:
            for a in out.values():
                self.host_register(a)
        return out

    def extend_candidates(self, q, r: float, robot_radius: float, cap: Optional[int] = None, out: Optional[dict] = None):
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        if out is not None:                      # caller-owned arrays (extend_out_buffers): no allocation, no growth
            cap = out["idx"].shape[0]
            needed = C.c_int64()
            self._check(self._lib.rrtx_extend_candidates(
                self._h, _capi._ptr(q), nq, r, robot_radius, _capi._ptr(out["offsets"]), _capi._ptr(out["idx"]),
                _capi._ptr(out["cost"]), _capi._ptr(out["hit_out"]), _capi._ptr(out["hit_in"]), cap, C.byref(needed),
                _capi._ptr(out["nearest_idx"]), _capi._ptr(out["nearest_dist"]), _capi._ptr(out["sample_unsafe"])))
            n = int(needed.value)
            return dict(offsets=out["offsets"], idx=out["idx"][:n], cost=out["cost"][:n], hit_out=out["hit_out"][:n],
                        hit_in=out["hit_in"][:n], nearest_idx=out["nearest_idx"], nearest_dist=out["nearest_dist"],
                        sample_unsafe=out["sample_unsafe"])
        if cap is None:
            cap = max(64 * nq, 1024)
        offsets = np.empty(nq + 1, dtype=np.int64)
        nidx = np.empty(nq, dtype=np.int32)
        ndist = np.empty(nq, dtype=np.float64)
        unsafe = np.empty(nq, dtype=np.uint8)

        def call(cap, needed):
            idx = np.empty(cap, dtype=np.int32)
            cost = np.empty(cap, dtype=np.float64)
            hout = np.empty(cap, dtype=np.uint8)
            hin = np.empty(cap, dtype=np.uint8)
            return self._lib.rrtx_extend_candidates(self._h, _capi._ptr(q), nq, r, robot_radius, _capi._ptr(offsets),
                                                    _capi._ptr(idx), _capi._ptr(cost), _capi._ptr(hout),
                                                    _capi._ptr(hin), cap, needed, _capi._ptr(nidx), _capi._ptr(ndist),
                                                    _capi._ptr(unsafe)), (idx, cost, hout, hin)
        n, (idx, cost, hout, hin) = self._two_call(cap, call)
        return dict(offsets=offsets, idx=idx[:n], cost=cost[:n], hit_out=hout[:n], hit_in=hin[:n],
                    nearest_idx=nidx, nearest_dist=ndist, sample_unsafe=unsafe)

    def extend_candidates_self(self, q, r: float, robot_radius: float, skip=None, cap: Optional[int] = None) -> dict:
        """rrtx_extend_candidates_self: the samples of one batch among themselves.  Row j of the CSR holds the batch
        positions i < j within r of sample j (ascending), with the SimpleEdge cost and the collision flags of
        q_j -> q_i (hit_out) and q_i -> q_j (hit_in).  skip: one byte per sample, non-zero = the sample has no list
        and is in none (the sample_unsafe bytes of extend_candidates serve as they are).  The tree is not read.
        dict(offsets, idx, cost, hit_out, hit_in); cap grows on demand."""
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
        if sk is not None and sk.shape[0] != nq:
            raise ValueError("skip needs one byte per sample")
        if cap is None:
            cap = max(8 * nq, 1024)
        offsets = np.empty(nq + 1, dtype=np.int64)

        def call(cap, needed):
            idx = np.empty(cap, dtype=np.int32)
            cost = np.empty(cap, dtype=np.float64)
            hout = np.empty(cap, dtype=np.uint8)
            hin = np.empty(cap, dtype=np.uint8)
            return self._lib.rrtx_extend_candidates_self(self._h, _capi._ptr(q), nq, r, robot_radius, _capi._ptr(sk),
                                                         _capi._ptr(offsets), _capi._ptr(idx), _capi._ptr(cost),
                                                         _capi._ptr(hout), _capi._ptr(hin), cap, needed), (idx, cost, hout, hin)
        n, (idx, cost, hout, hin) = self._two_call(cap, call)
        return dict(offsets=offsets, idx=idx[:n], cost=cost[:n], hit_out=hout[:n], hit_in=hin[:n])

    def extend_closest_self(self, q, k: int, robot_radius: float, skip=None, want=None, tree_idx=None) -> dict:
        """rrtx_extend_closest_self: for the closestNode rule of a batch.  Row j (of k slots) holds the nearest live
        earlier samples i < j of the batch ordered by (distance, i), with the SimpleEdge cost and the flags of
        q_j -> q_i (hit_out) and q_i -> q_j (hit_in) against the whole obstacle list; count[j] of them are used, the
        other slots have idx -1, cost +Inf.  skip: non-zero bytes take a sample out (sample_unsafe of
        extend_candidates); want: non-zero bytes choose the rows to fill (None: every live row); tree_idx: one node
        per sample whose two flags come back as tree_hit_out / tree_hit_in (an index outside the tree gives 0).
        dict(idx, cost, hit_out, hit_in: (nq, k); count: (nq,); tree_hit_out, tree_hit_in: (nq,) or None)."""
        q = f64(q, (-1, self.dim))
        nq, k = q.shape[0], int(k)

        def per_sample(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if a.shape[0] != nq:
                raise ValueError(what + " needs one entry per sample")
            return a
        sk, wa = per_sample(skip, np.uint8, "skip"), per_sample(want, np.uint8, "want")
        ti = per_sample(tree_idx, np.int32, "tree_idx")
        rows = max(k, 0)
        idx = np.empty((nq, rows), dtype=np.int32)
        cost = np.empty((nq, rows), dtype=np.float64)
        hout = np.empty((nq, rows), dtype=np.uint8)
        hin = np.empty((nq, rows), dtype=np.uint8)
        count = np.empty(nq, dtype=np.int32)
        tho = None if ti is None else np.empty(nq, dtype=np.uint8)
        thi = None if ti is None else np.empty(nq, dtype=np.uint8)
        self._check(self._lib.rrtx_extend_closest_self(self._h, _capi._ptr(q), nq, k, robot_radius, _capi._ptr(sk),
                                                       _capi._ptr(wa), _capi._ptr(ti), _capi._ptr(idx), _capi._ptr(cost),
                                                       _capi._ptr(hout), _capi._ptr(hin), _capi._ptr(count),
                                                       _capi._ptr(tho), _capi._ptr(thi)))
        return dict(idx=idx, cost=cost, hit_out=hout, hit_in=hin, count=count, tree_hit_out=tho, tree_hit_in=thi)

    # ---- findBestParent + rewire test on the device -------------------------------------------------
    def node_cost_set(self, first_index: int, lmc):
        """rrtLMC of nodes first_index .. first_index + len(lmc) - 1 in the context's own device array (+Inf for a node
        never set); extend_select(lmc=None) reads it."""
        v = f64(lmc, (-1,))
        self._check(self._lib.rrtx_node_cost_set(self._h, int(first_index), _capi._ptr(v), v.shape[0]))

    def select_out_buffers(self, nq: int, rw_cap: int, register: bool = False, list_cap: int = 0,
                           dubins: bool = False) -> dict:
        """Output arrays for extend_select(..., out=...) that a caller keeps across calls.  register=True page-locks
        them; the context keeps them alive and unregisters them in close().  list_cap > 0 adds room for the neighbour
        lists themselves (a planner that keeps RRT^X neighbour sets); dubins: the three double columns of
        extend_select_dubins instead of the one cost column."""
        out = dict(parent_idx=np.empty(nq, dtype=np.int32), parent_entry=np.empty(nq, dtype=np.int64),
                   lmc_new=np.empty(nq, dtype=np.float64), status=np.empty(nq, dtype=np.uint8),
                   rw_offsets=np.empty(nq + 1, dtype=np.int64), rw_node=np.empty(max(rw_cap, 1), dtype=np.int32),
                   rw_value=np.empty(max(rw_cap, 1), dtype=np.float64), nearest_idx=np.empty(nq, dtype=np.int32),
                   nearest_dist=np.empty(nq, dtype=np.float64), sample_unsafe=np.empty(nq, dtype=np.uint8))
        if list_cap > 0:
            out.update(offsets=np.empty(nq + 1, dtype=np.int64), idx=np.empty(list_cap, dtype=np.int32),
                       hit_out=np.empty(list_cap, dtype=np.uint8), hit_in=np.empty(list_cap, dtype=np.uint8))
            out.update({k: np.empty(list_cap, dtype=np.float64)
                        for k in (("key", "cost_out", "cost_in") if dubins else ("cost",))})
        if register:
            for a in out.values():
                if a.nbytes:
                    self.host_register(a)
                    self._registered.append(a)
        return out

    def extend_select(self, q, r: float, robot_radius: float, lmc=None, rw_cap: Optional[int] = None,
                      out: Optional[dict] = None, want_lists: bool = False, cap: Optional[int] = None):
        """rrtx_extend_select: per sample the parent findBestParent picks, the sample's rrtLMC, a status
        (_capi.RRTX_SEL_*) and the neighbours the rewire test of extend() would lower, as a CSR (rw_offsets, rw_node,
        rw_value).  lmc: rrtLMC of every node, or None for the values node_cost_set left on the device.
        out: arrays of select_out_buffers (no allocation, no growth: a count beyond their room raises
        RRTX_E_CAPACITY); otherwise the arrays are allocated here and grown on demand.  want_lists also returns
        the neighbour lists (offsets, idx, cost, hit_out, hit_in)."""
        return self._extend_select(self._lib.rrtx_extend_select, q, (r, robot_radius), ("cost",), lmc, rw_cap, out,
                                   want_lists, cap)

    def extend_select_dubins(self, q, r: float, robot_radius: float, r_min: float, lmc=None,
                             rw_cap: Optional[int] = None, out: Optional[dict] = None, want_lists: bool = False,
                             cap: Optional[int] = None):
        """rrtx_extend_select_dubins: extend_select for a dim=4 [x y t theta] context (wraps, time, the polygon list as
        in extend_candidates_dubins).  want_lists returns offsets, idx, key, cost_out, cost_in, hit_out, hit_in.  The
        lists stay on the device for graph_edges_append_selected, which links them with their two cost columns."""
        return self._extend_select(self._lib.rrtx_extend_select_dubins, q, (r, robot_radius, r_min),
                                   ("key", "cost_out", "cost_in"), lmc, rw_cap, out, want_lists, cap)

    def _extend_select(self, fn, q, scalars, cols, lmc, rw_cap, out, want_lists, cap):
        # (the two select calls differ in their scalars and in the double columns of their lists, `cols`)
        q = f64(q, (-1, self.dim))
        nq = q.shape[0]
        lmc_a = None if lmc is None else f64(lmc, (-1,))
        if lmc_a is not None and lmc_a.shape[0] < self.n_nodes:
            raise ValueError("lmc needs one entry per node")
        fixed = out is not None
        if fixed:
            rw_cap = out["rw_node"].shape[0]
            want_lists = "idx" in out
            cap = out["idx"].shape[0] if want_lists else 0
        else:
            out = self.select_out_buffers(nq, 0)
            rw_cap = max(16 * nq, 1024) if rw_cap is None else int(rw_cap)
            cap = (max(64 * nq, 1024) if cap is None else int(cap)) if want_lists else 0
            if want_lists:
                out["offsets"] = np.empty(nq + 1, dtype=np.int64)
        while True:
            if not fixed:
                if out["rw_node"].shape[0] < max(rw_cap, 1):
                    out["rw_node"] = np.empty(max(rw_cap, 1), dtype=np.int32)
                    out["rw_value"] = np.empty(max(rw_cap, 1), dtype=np.float64)
                if want_lists and ("idx" not in out or out["idx"].shape[0] < max(cap, 1)):
                    out.update(idx=np.empty(max(cap, 1), dtype=np.int32), hit_out=np.empty(max(cap, 1), dtype=np.uint8),
                               hit_in=np.empty(max(cap, 1), dtype=np.uint8))
                    out.update({k: np.empty(max(cap, 1), dtype=np.float64) for k in cols})
            rw_needed, needed = C.c_int64(), C.c_int64()
            g = (lambda k: _capi._ptr(out[k])) if want_lists else (lambda k: None)
            rc = fn(
                self._h, _capi._ptr(q), nq, *scalars, _capi._ptr(lmc_a), _capi._ptr(out["parent_idx"]),
                _capi._ptr(out["parent_entry"]), _capi._ptr(out["lmc_new"]), _capi._ptr(out["status"]),
                _capi._ptr(out["rw_offsets"]), _capi._ptr(out["rw_node"]), _capi._ptr(out["rw_value"]), rw_cap,
                C.byref(rw_needed), _capi._ptr(out["nearest_idx"]), _capi._ptr(out["nearest_dist"]),
                _capi._ptr(out["sample_unsafe"]), g("offsets"), g("idx"), *[g(k) for k in cols], g("hit_out"), g("hit_in"),
                cap, C.byref(needed))
            if rc != _capi.RRTX_E_CAPACITY or fixed:
                self._check(rc)
                break
            rw_cap = max(rw_cap, int(rw_needed.value))
            cap = max(cap, int(needed.value)) if want_lists else 0
        nrw, n = int(rw_needed.value), int(needed.value)
        res = {k: out[k] for k in ("parent_idx", "parent_entry", "lmc_new", "status", "rw_offsets", "nearest_idx",
                                   "nearest_dist", "sample_unsafe")}
        res.update(rw_node=out["rw_node"][:nrw], rw_value=out["rw_value"][:nrw], n_neighbors=n)
        if want_lists:
            res.update(offsets=out["offsets"], idx=out["idx"][:n], hit_out=out["hit_out"][:n], hit_in=out["hit_in"][:n])
            res.update({k: out[k][:n] for k in cols})
        return res

    def extend_select_dev(self, nq: int, offsets_ptr: int, idx_ptr: int, cost_out_ptr: int, cost_in_ptr: int,
                          hit_out_ptr: int, hit_in_ptr: int, n_valid_ptr: Optional[int], cap: int,
                          unsafe_ptr: Optional[int], lmc_ptr: Optional[int], parent_idx_ptr: int, parent_entry_ptr: int,
                          lmc_new_ptr: int, status_ptr: int, rw_offsets_ptr: int, rw_node_ptr: int, rw_value_ptr: int,
                          rw_cap: int, rw_needed_ptr: int):
        """rrtx_extend_select_dev over the device lists of extend_candidates_dev / extend_candidates_dubins_dev (for
        SimpleEdge lists pass the cost array twice); lmc_ptr None selects the array node_cost_set fills."""
        self._check(self._lib.rrtx_extend_select_dev(
            self._h, nq, offsets_ptr, idx_ptr, cost_out_ptr, cost_in_ptr, hit_out_ptr, hit_in_ptr, n_valid_ptr, cap,
            unsafe_ptr, lmc_ptr, parent_idx_ptr, parent_entry_ptr, lmc_new_ptr, status_ptr, rw_offsets_ptr, rw_node_ptr,
            rw_value_ptr, rw_cap, rw_needed_ptr))

    # ---- findNewTarget on the device ----------------------------------------------------------------
    def _find_new_target(self, pose, r0, r_max: float, robot_radius: float, lmc, r_min):
        pose = f64(pose, (-1, self.dim))
        nq = pose.shape[0]
        r = f64(r0, (-1,))
        if r.shape[0] not in (1, nq):
            raise ValueError("r0 must be a scalar or have one entry per pose")
        stride = 0 if r.shape[0] == 1 else 1
        lmc_a = None if lmc is None else f64(lmc, (-1,))
        if lmc_a is not None and lmc_a.shape[0] < self.n_nodes:
            raise ValueError("lmc needs one entry per node")
        out = dict(target_idx=np.empty(nq, dtype=np.int32), edge_dist=np.empty(nq, dtype=np.float64),
                   cost_to_goal=np.empty(nq, dtype=np.float64), radius_used=np.empty(nq, dtype=np.float64),
                   rounds=np.empty(nq, dtype=np.int32), status=np.empty(nq, dtype=np.uint8))
        tail = [_capi._ptr(lmc_a)] + [_capi._ptr(out[k]) for k in ("target_idx", "edge_dist", "cost_to_goal", "radius_used",
                                                                    "rounds", "status")]
        head = [self._h, _capi._ptr(pose), nq, _capi._ptr(r), stride, float(r_max), float(robot_radius)]
        if r_min is None:
            self._check(self._lib.rrtx_find_new_target(*head, *tail))
        else:
            self._check(self._lib.rrtx_find_new_target_dubins(*head, float(r_min), *tail))
        return out

    def find_new_target(self, pose, r0, r_max: float, robot_radius: float, lmc=None) -> dict:
        """rrtx_find_new_target (SimpleEdge, dim 3): per pose the neighbour with the lowest rrtLMC + edge.dist over the
        safe edges pose -> neighbour, the ball doubling from r0 (a scalar or one radius per pose) until one exists or it
        exceeds r_max.  dict(target_idx, edge_dist, cost_to_goal, radius_used, rounds, status); status is
        _capi.RRTX_TGT_OK or RRTX_TGT_NOT_FOUND.  lmc: rrtLMC of every node, or None for what node_cost_set left on the
        device."""
        return self._find_new_target(pose, r0, r_max, robot_radius, lmc, None)

    def find_new_target_dubins(self, pose, r0, r_max: float, robot_radius: float, r_min: float, lmc=None) -> dict:
        """rrtx_find_new_target_dubins (dim 4, [x y t theta], polygon list; wraps and a space with time as set)."""
        return self._find_new_target(pose, r0, r_max, robot_radius, lmc, r_min)

    def extend_candidates_dubins(self, q, r: float, robot_radius: float, r_min: float, cap: Optional[int] = None):
        """Fused extend() preamble for Edge = DubinsEdge (dim 4, theta wrapped, polygon obstacles)."""
        q = f64(q, (-1, 4))
        nq = q.shape[0]
        if cap is None:
            cap = max(256 * nq, 1024)
        offsets = np.empty(nq + 1, dtype=np.int64)
        nidx = np.empty(nq, dtype=np.int32)
        ndist = np.empty(nq, dtype=np.float64)
        unsafe = np.empty(nq, dtype=np.uint8)

        def call(cap, needed):
            idx = np.empty(cap, dtype=np.int32)
            key = np.empty(cap, dtype=np.float64)
            co = np.empty(cap, dtype=np.float64)
            ci = np.empty(cap, dtype=np.float64)
            wo = np.empty((cap, 3), dtype=np.uint8)
            wi = np.empty((cap, 3), dtype=np.uint8)
            ho = np.empty(cap, dtype=np.uint8)
            hi = np.empty(cap, dtype=np.uint8)
            return self._lib.rrtx_extend_candidates_dubins(
                self._h, _capi._ptr(q), nq, r, robot_radius, r_min, _capi._ptr(offsets), _capi._ptr(idx),
                _capi._ptr(key), _capi._ptr(co), _capi._ptr(ci), _capi._ptr(wo), _capi._ptr(wi), _capi._ptr(ho),
                _capi._ptr(hi), cap, needed, _capi._ptr(nidx), _capi._ptr(ndist),
                _capi._ptr(unsafe)), (idx, key, co, ci, wo, wi, ho, hi)
        n, (idx, key, co, ci, wo, wi, ho, hi) = self._two_call(cap, call)
        return dict(offsets=offsets, idx=idx[:n], key=key[:n], cost_out=co[:n], cost_in=ci[:n],
                    word_out=wo[:n].view("S3").ravel(), word_in=wi[:n].view("S3").ravel(), hit_out=ho[:n],
                    hit_in=hi[:n], nearest_idx=nidx, nearest_dist=ndist, sample_unsafe=unsafe)

    def extend_candidates_self_dubins(self, q, r: float, robot_radius: float, r_min: float, skip=None,
                                      cap: Optional[int] = None) -> dict:
        """rrtx_extend_candidates_self_dubins: the samples of one Dubins batch among themselves (dim 4, the wrapped
        dimensions as set).  Row j of the CSR holds the batch positions i < j that a copy of sample j reaches within r
        (ascending), with the key of the first such copy and the Dubins cost, word and flags of q_j -> q_i (out) and
        q_i -> q_j (in), as extend_candidates_dubins reports them.  skip: one byte per sample, non-zero = the sample has
        no list and is in none (the sample_unsafe bytes of extend_candidates_dubins serve as they are).  The tree is
        not read.  dict(offsets, idx, key, cost_out, cost_in, word_out, word_in, hit_out, hit_in); cap grows on demand."""
        q = f64(q, (-1, 4))
        nq = q.shape[0]
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
        if sk is not None and sk.shape[0] != nq:
            raise ValueError("skip needs one byte per sample")
        if cap is None:
            cap = max(8 * nq, 1024)
        offsets = np.empty(nq + 1, dtype=np.int64)

        def call(cap, needed):
            idx = np.empty(cap, dtype=np.int32)
            key = np.empty(cap, dtype=np.float64)
            co = np.empty(cap, dtype=np.float64)
            ci = np.empty(cap, dtype=np.float64)
            wo = np.empty((cap, 3), dtype=np.uint8)
            wi = np.empty((cap, 3), dtype=np.uint8)
            ho = np.empty(cap, dtype=np.uint8)
            hi = np.empty(cap, dtype=np.uint8)
            return self._lib.rrtx_extend_candidates_self_dubins(
                self._h, _capi._ptr(q), nq, r, robot_radius, r_min, _capi._ptr(sk), _capi._ptr(offsets), _capi._ptr(idx),
                _capi._ptr(key), _capi._ptr(co), _capi._ptr(ci), _capi._ptr(wo), _capi._ptr(wi), _capi._ptr(ho),
                _capi._ptr(hi), cap, needed), (idx, key, co, ci, wo, wi, ho, hi)
        n, (idx, key, co, ci, wo, wi, ho, hi) = self._two_call(cap, call)
        return dict(offsets=offsets, idx=idx[:n], key=key[:n], cost_out=co[:n], cost_in=ci[:n],
                    word_out=wo[:n].view("S3").ravel(), word_in=wi[:n].view("S3").ravel(), hit_out=ho[:n], hit_in=hi[:n])

    def extend_closest_self_dubins(self, q, k: int, robot_radius: float, r_min: float, skip=None, want=None,
                                   tree_idx=None) -> dict:
        """rrtx_extend_closest_self_dubins: for the closestNode rule of a Dubins batch (dim 4, the wrapped dimensions as
        set).  Row j (of k slots) holds the nearest live earlier samples i < j of the batch ordered by (s, i), s the
        minimum over the copies of q_j of the squared distance to q_i, with key = sqrt(s) and the Dubins cost, word and
        flags of q_j -> q_i (out) and q_i -> q_j (in) against the whole polygon list; count[j] of them are used, the other
        slots have idx -1, key and costs +Inf.  skip: non-zero bytes take a sample out (sample_unsafe of
        extend_candidates_dubins); want: non-zero bytes choose the rows to fill (None: every live row); tree_idx: one node
        per sample whose fields come back as tree_cost_out, tree_cost_in, tree_word_out, tree_word_in, tree_hit_out,
        tree_hit_in (an index outside the tree gives +Inf and 0).
        dict(idx, key, cost_out, cost_in, word_out, word_in, hit_out, hit_in: (nq, k); count: (nq,); tree_*: (nq,) or
        None)."""
        q = f64(q, (-1, 4))
        nq, k = q.shape[0], int(k)

        def per_sample(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if a.shape[0] != nq:
                raise ValueError(what + " needs one entry per sample")
            return a
        sk, wa = per_sample(skip, np.uint8, "skip"), per_sample(want, np.uint8, "want")
        ti = per_sample(tree_idx, np.int32, "tree_idx")
        rows = max(k, 0)
        idx = np.empty((nq, rows), dtype=np.int32)
        key, co, ci = (np.empty((nq, rows), dtype=np.float64) for _ in range(3))
        wo, wi = (np.empty((nq, rows, 3), dtype=np.uint8) for _ in range(2))
        ho, hi = (np.empty((nq, rows), dtype=np.uint8) for _ in range(2))
        count = np.empty(nq, dtype=np.int32)
        tco = tci = two = twi = tho = thi = None
        if ti is not None:
            tco, tci = (np.empty(nq, dtype=np.float64) for _ in range(2))
            two, twi = (np.empty((nq, 3), dtype=np.uint8) for _ in range(2))
            tho, thi = (np.empty(nq, dtype=np.uint8) for _ in range(2))
        self._check(self._lib.rrtx_extend_closest_self_dubins(
            self._h, _capi._ptr(q), nq, k, robot_radius, r_min, _capi._ptr(sk), _capi._ptr(wa), _capi._ptr(ti),
            _capi._ptr(idx), _capi._ptr(key), _capi._ptr(co), _capi._ptr(ci), _capi._ptr(wo), _capi._ptr(wi), _capi._ptr(ho),
            _capi._ptr(hi), _capi._ptr(count), _capi._ptr(tco), _capi._ptr(tci), _capi._ptr(two), _capi._ptr(twi),
            _capi._ptr(tho), _capi._ptr(thi)))

        def words(w, shape):
            return None if w is None else w.view("S3").reshape(shape)
        return dict(idx=idx, key=key, cost_out=co, cost_in=ci, word_out=words(wo, (nq, rows)), word_in=words(wi, (nq, rows)),
                    hit_out=ho, hit_in=hi, count=count, tree_cost_out=tco, tree_cost_in=tci,
                    tree_word_out=words(two, (nq,)), tree_word_in=words(twi, (nq,)), tree_hit_out=tho, tree_hit_in=thi)

    # ---- device-pointer variants (pointers are ints, e.g. torch.Tensor.data_ptr()) ----------------
    def nn_nearest_dev(self, q_ptr: int, nq: int, idx_ptr: int, dist_ptr: int):
        self._check(self._lib.rrtx_nn_nearest_dev(self._h, q_ptr, nq, idx_ptr, dist_ptr))

    def nn_knearest_dev(self, q_ptr: int, nq: int, k: int, idx_ptr: int, dist_ptr: int, count_ptr: int):
        self._check(self._lib.rrtx_nn_knearest_dev(self._h, q_ptr, nq, k, idx_ptr, dist_ptr, count_ptr))

    def nn_radius_dev(self, q_ptr: int, r: float, nq: int, offsets_ptr: int, idx_ptr: int, dist_ptr: int, cap: int,
                      needed_ptr: int):
        self._check(self._lib.rrtx_nn_radius_dev(self._h, q_ptr, r, nq, offsets_ptr, idx_ptr, dist_ptr, cap,
                                                 needed_ptr))

    def edges_check_dev(self, kind: int, p0_ptr: int, p1_ptr: int, ne: int, robot_radius: float, obstacle: int,
                        obs_begin: int, obs_end: int, hit_ptr: int, first_ptr: Optional[int]):
        self._check(self._lib.rrtx_edges_check_dev(self._h, kind, p0_ptr, p1_ptr, ne, robot_radius, obstacle,
                                                   obs_begin, obs_end, hit_ptr, first_ptr))

    def points_check_dev(self, kind: int, p_ptr: int, n: int, robot_radius: float, quick: bool, unsafe_ptr: int,
                         clr_ptr: Optional[int]):
        self._check(self._lib.rrtx_points_check_dev(self._h, kind, p_ptr, n, robot_radius, 1 if quick else 0,
                                                    unsafe_ptr, clr_ptr))

    def extend_candidates_dev(self, q_ptr: int, nq: int, r: float, robot_radius: float, offsets_ptr: int,
                              idx_ptr: int, cost_ptr: int, hit_out_ptr: int, hit_in_ptr: int, cap: int,
                              needed_ptr: int, nearest_idx_ptr: Optional[int] = None,
                              nearest_dist_ptr: Optional[int] = None, unsafe_ptr: Optional[int] = None):
        self._check(self._lib.rrtx_extend_candidates_dev(self._h, q_ptr, nq, r, robot_radius, offsets_ptr, idx_ptr,
                                                         cost_ptr, hit_out_ptr, hit_in_ptr, cap, needed_ptr,
                                                         nearest_idx_ptr, nearest_dist_ptr, unsafe_ptr))

    def extend_candidates_self_dev(self, q_ptr: int, nq: int, r: float, robot_radius: float, skip_ptr: Optional[int],
                                   offsets_ptr: int, idx_ptr: int, cost_ptr: int, hit_out_ptr: int, hit_in_ptr: int,
                                   cap: int, needed_ptr: int):
        self._check(self._lib.rrtx_extend_candidates_self_dev(self._h, q_ptr, nq, r, robot_radius, skip_ptr, offsets_ptr,
                                                              idx_ptr, cost_ptr, hit_out_ptr, hit_in_ptr, cap, needed_ptr))

    def extend_closest_self_dev(self, q_ptr: int, nq: int, k: int, robot_radius: float, skip_ptr: Optional[int],
                                want_ptr: Optional[int], tree_idx_ptr: Optional[int], idx_ptr: int, cost_ptr: int,
                                hit_out_ptr: int, hit_in_ptr: int, count_ptr: int,
                                tree_hit_out_ptr: Optional[int] = None, tree_hit_in_ptr: Optional[int] = None):
        self._check(self._lib.rrtx_extend_closest_self_dev(self._h, q_ptr, nq, k, robot_radius, skip_ptr, want_ptr,
                                                           tree_idx_ptr, idx_ptr, cost_ptr, hit_out_ptr, hit_in_ptr,
                                                           count_ptr, tree_hit_out_ptr, tree_hit_in_ptr))

    def extend_candidates_dubins_dev(self, q_ptr: int, nq: int, r: float, robot_radius: float, r_min: float,
                                     offsets_ptr: int, idx_ptr: int, key_ptr: int, cost_out_ptr: int, cost_in_ptr: int,
                                     word_out_ptr: Optional[int], word_in_ptr: Optional[int], hit_out_ptr: int,
                                     hit_in_ptr: int, cap: int, needed_ptr: int, nearest_idx_ptr: Optional[int] = None,
                                     nearest_dist_ptr: Optional[int] = None, unsafe_ptr: Optional[int] = None):
        self._check(self._lib.rrtx_extend_candidates_dubins_dev(
            self._h, q_ptr, nq, r, robot_radius, r_min, offsets_ptr, idx_ptr, key_ptr, cost_out_ptr, cost_in_ptr,
            word_out_ptr, word_in_ptr, hit_out_ptr, hit_in_ptr, cap, needed_ptr, nearest_idx_ptr, nearest_dist_ptr,
            unsafe_ptr))

    def extend_candidates_self_dubins_dev(self, q_ptr: int, nq: int, r: float, robot_radius: float, r_min: float,
                                          skip_ptr: Optional[int], offsets_ptr: int, idx_ptr: int, key_ptr: int,
                                          cost_out_ptr: int, cost_in_ptr: int, word_out_ptr: Optional[int],
                                          word_in_ptr: Optional[int], hit_out_ptr: int, hit_in_ptr: int, cap: int,
                                          needed_ptr: int):
        self._check(self._lib.rrtx_extend_candidates_self_dubins_dev(
            self._h, q_ptr, nq, r, robot_radius, r_min, skip_ptr, offsets_ptr, idx_ptr, key_ptr, cost_out_ptr, cost_in_ptr,
            word_out_ptr, word_in_ptr, hit_out_ptr, hit_in_ptr, cap, needed_ptr))

    def extend_closest_self_dubins_dev(self, q_ptr: int, nq: int, k: int, robot_radius: float, r_min: float,
                                       skip_ptr: Optional[int], want_ptr: Optional[int], tree_idx_ptr: Optional[int],
                                       idx_ptr: int, key_ptr: int, cost_out_ptr: int, cost_in_ptr: int,
                                       word_out_ptr: Optional[int], word_in_ptr: Optional[int], hit_out_ptr: int,
                                       hit_in_ptr: int, count_ptr: int, tree_cost_out_ptr: Optional[int] = None,
                                       tree_cost_in_ptr: Optional[int] = None, tree_word_out_ptr: Optional[int] = None,
                                       tree_word_in_ptr: Optional[int] = None, tree_hit_out_ptr: Optional[int] = None,
                                       tree_hit_in_ptr: Optional[int] = None):
        self._check(self._lib.rrtx_extend_closest_self_dubins_dev(
            self._h, q_ptr, nq, k, robot_radius, r_min, skip_ptr, want_ptr, tree_idx_ptr, idx_ptr, key_ptr, cost_out_ptr,
            cost_in_ptr, word_out_ptr, word_in_ptr, hit_out_ptr, hit_in_ptr, count_ptr, tree_cost_out_ptr, tree_cost_in_ptr,
            tree_word_out_ptr, tree_word_in_ptr, tree_hit_out_ptr, tree_hit_in_ptr))

    def pack_hits_dev(self, hit_out_ptr: int, hit_in_ptr: int, n_valid_ptr: int, cap: int, words_ptr: int):
        self._check(self._lib.rrtx_pack_hits_dev(self._h, hit_out_ptr, hit_in_ptr, n_valid_ptr, cap, words_ptr))

    # ---- obstacle sweeps over the device mirror of the planner's edges ----------------
    def graph_edges_append(self, start_idx, end_idx) -> int:
        a = np.ascontiguousarray(start_idx, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(end_idx, dtype=np.int32).reshape(-1)
        assert a.shape == b.shape
        first = C.c_int64()
        self._check(self._lib.rrtx_graph_edges_append(self._h, _capi._ptr(a), _capi._ptr(b), a.shape[0], C.byref(first)))
        return first.value

    @property
    def n_graph_edges(self) -> int:
        return int(self._lib.rrtx_graph_edges_count(self._h))

    def graph_edges_clear(self):
        self._check(self._lib.rrtx_graph_edges_clear(self._h))

    def graph_edges_set_dist(self, first_id: int, dist):
        """edge.dist of mirrored edges [first_id, first_id + len(dist)) (Inf = blocked)"""
        d = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        self._check(self._lib.rrtx_graph_edges_set_dist(self._h, int(first_id), _capi._ptr(d), d.shape[0]))

    def graph_edges_block(self, edge_ids):
        """addNewObstacle's `edge.dist = Inf` for the ids an obstacle sweep returned"""
        self._edge_ids_call(self._lib.rrtx_graph_edges_block, edge_ids)

    def graph_edges_unblock(self, edge_ids):
        """removeObstacle's `edge.dist = edge.distOriginal` for the ids a release returned: the cost append / set_dist
        wrote last comes back (an id that is not blocked keeps its value)"""
        self._edge_ids_call(self._lib.rrtx_graph_edges_unblock, edge_ids)

    # ---- the extend lists become mirror edges on the device (include/rrtx.h, "the extend lists become mirror edges")
    def graph_edges_append_lists(self, offsets, idx, cost_out, cost_in, hit_out, hit_in, node_of, idx_is_batch: bool = False,
                                 n_valid: Optional[int] = None, cap: Optional[int] = None, want_rows: bool = True):
        """rrtx_graph_edges_append_lists over host arrays: per inserted sample j (node_of[j] >= 0) and surviving entry the
        out-edge node_of[j] -> near (blocked when hit_out != 0) and, when hit_in == 0, the in-edge.  cost_in may be the
        same array as cost_out (SimpleEdge).  Returns (first_id, n_added, row_first or None)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        nq = off.shape[0] - 1 if off.shape[0] else 0
        ia = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        co = f64(cost_out, (-1,))
        ci = co if cost_in is cost_out else f64(cost_in, (-1,))
        ho = np.ascontiguousarray(hit_out, dtype=np.uint8).reshape(-1)
        hi = np.ascontiguousarray(hit_in, dtype=np.uint8).reshape(-1)
        nd = np.ascontiguousarray(node_of, dtype=np.int32).reshape(-1)
        if nd.shape[0] != nq:
            raise ValueError("node_of needs one entry per sample")
        room = min(ia.shape[0], co.shape[0], ci.shape[0], ho.shape[0], hi.shape[0])
        cap = room if cap is None else int(cap)
        if cap > room:
            raise ValueError("cap exceeds the list arrays")
        n_valid = (int(off[nq]) if nq else 0) if n_valid is None else int(n_valid)
        rows = np.empty(nq + 1, dtype=np.int64) if want_rows else None
        first, added = C.c_int64(), C.c_int64()
        self._check(self._lib.rrtx_graph_edges_append_lists(
            self._h, nq, _capi._ptr(off), _capi._ptr(ia), _capi._ptr(co), _capi._ptr(ci), _capi._ptr(ho), _capi._ptr(hi),
            n_valid, cap, _capi._ptr(nd), 1 if idx_is_batch else 0, C.byref(first), C.byref(added), _capi._ptr(rows)))
        return first.value, added.value, rows

    def graph_edges_append_lists_dev(self, nq: int, offsets_ptr: int, idx_ptr: int, cost_out_ptr: int, cost_in_ptr: int,
                                     hit_out_ptr: int, hit_in_ptr: int, n_valid_ptr: Optional[int], cap: int,
                                     node_of_ptr: int, idx_is_batch: bool = False, row_first_ptr: Optional[int] = None):
        """rrtx_graph_edges_append_lists_dev over device lists (those of extend_candidates_dev and its kin); waits on the
        stream once for the counts.  Returns (first_id, n_added); row_first_ptr: nq + 1 int64 on the device, or None."""
        first, added = C.c_int64(), C.c_int64()
        self._check(self._lib.rrtx_graph_edges_append_lists_dev(
            self._h, nq, offsets_ptr, idx_ptr, cost_out_ptr, cost_in_ptr, hit_out_ptr, hit_in_ptr, n_valid_ptr, cap,
            node_of_ptr, 1 if idx_is_batch else 0, C.byref(first), C.byref(added), row_first_ptr))
        return first.value, added.value

    def graph_edges_append_selected(self, node_of, want_rows: bool = True):
        """rrtx_graph_edges_append_selected: the same over the lists the last extend_select left on the device
        (RRTX_E_STATE when another call has used their workspaces since, or node_of has another length).
        Returns (first_id, n_added, row_first or None)."""
        nd = np.ascontiguousarray(node_of, dtype=np.int32).reshape(-1)
        nq = nd.shape[0]
        rows = np.empty(nq + 1, dtype=np.int64) if want_rows else None
        first, added = C.c_int64(), C.c_int64()
        self._check(self._lib.rrtx_graph_edges_append_selected(self._h, nq, _capi._ptr(nd), C.byref(first), C.byref(added),
                                                               _capi._ptr(rows)))
        return first.value, added.value, rows

    def graph_edges_get(self, ids=None, first_id: int = 0, n: Optional[int] = None):
        """rrtx_graph_edges_get: (start, end, dist, dist_original) of the mirror edges `ids`, or of the range
        [first_id, first_id + n) (n None: to the end of the mirror)."""
        if ids is not None:
            ia = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            n = ia.shape[0]
        else:
            ia = None
            n = self.n_graph_edges - int(first_id) if n is None else int(n)
        m = max(n, 0)
        start, end = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        dist, dist0 = np.empty(m, dtype=np.float64), np.empty(m, dtype=np.float64)
        self._check(self._lib.rrtx_graph_edges_get(self._h, _capi._ptr(ia), int(first_id), n, _capi._ptr(start),
                                                   _capi._ptr(end), _capi._ptr(dist), _capi._ptr(dist0)))
        return start, end, dist, dist0

    def graph_edges_cull(self, ball: float, nodes=None) -> int:
        """rrtx_graph_edges_cull: cullCurrentNeighbors(node, ball) over the mirror for the nodes listed (None: every
        node) -- every edge with start listed, start < end and dist > ball becomes culled (dist = distOriginal = +Inf,
        touched for the next cost update).  Returns the number of edges this call culled."""
        culled = C.c_int64()
        if nodes is None:
            ia, k = None, 0
        else:
            given = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
            k = given.shape[0]
            ia = given if k else np.zeros(1, dtype=np.int32)      # (an empty list is still a list: a pointer that is not NULL)
        self._check(self._lib.rrtx_graph_edges_cull(self._h, float(ball), _capi._ptr(ia), k, C.byref(culled)))
        return culled.value

    def graph_edges_compact(self, want_remap: bool = True):
        """rrtx_graph_edges_compact: the culled edges leave the mirror, survivors keep their order.  Returns
        (remap or None, n_removed): remap[old id] = new id, -1 for a removed edge.  RRTX_E_STATE when a kept cost solve
        still uses a culled edge as a parent edge (run graph_cost_update first)."""
        ne = self.n_graph_edges
        remap = np.empty(ne, dtype=np.int32) if want_remap else None
        removed = C.c_int64()
        self._check(self._lib.rrtx_graph_edges_compact(self._h, _capi._ptr(remap) if ne else None, ne, C.byref(removed)))
        return remap, removed.value

    def graph_edges_culled(self, first_id: int = 0, n: Optional[int] = None) -> np.ndarray:
        """rrtx_graph_edges_get_culled: one byte per edge of [first_id, first_id + n) (n None: to the end of the mirror),
        1 = culled"""
        n = self.n_graph_edges - int(first_id) if n is None else int(n)
        out = np.empty(max(n, 0), dtype=np.uint8)
        self._check(self._lib.rrtx_graph_edges_get_culled(self._h, int(first_id), n, _capi._ptr(out)))
        return out

    def _edge_ids_call(self, fn, edge_ids):
        ids = np.ascontiguousarray(edge_ids, dtype=np.int32).reshape(-1)
        self._check(fn(self._h, _capi._ptr(ids), ids.shape[0]))

    def graph_cost_to_root(self, root_idx: int, want_parent: bool = True, update: bool = False):
        """rrtLMC of every node at the fixed point of rewire / reduceInconsistency (changeThresh = 0) over the
        edge mirror, and the id of each node's parent edge (-1: root or orphan).  Returns (lmc, parent_edge, passes).
        update=True continues from the previous solve (rrtx_graph_cost_update): same answer, less work."""
        n = self.n_nodes
        lmc = np.empty(n, dtype=np.float64)
        par = np.empty(n, dtype=np.int32) if want_parent else None
        passes = C.c_int32()
        fn = self._lib.rrtx_graph_cost_update if update else self._lib.rrtx_graph_cost_to_root
        self._check(fn(self._h, int(root_idx), _capi._ptr(lmc), _capi._ptr(par) if want_parent else None, C.byref(passes)))
        return lmc, par, passes.value

    def graph_cost_update(self, root_idx: int, want_parent: bool = True):
        return self.graph_cost_to_root(root_idx, want_parent, update=True)

    def graph_cost_update_delta(self, root_idx: int, store: bool = False, cap: Optional[int] = None):
        """rrtx_graph_cost_update_delta: graph_cost_update's solve, reported as the nodes whose rrtLMC (bit pattern) or
        parent edge differs from what this call last reported for the root (a node never reported counts as +Inf / -1).
        Returns (node, lmc, parent_edge, passes), nodes ascending; lmc +Inf and parent_edge -1 for a new orphan.
        store=True also leaves the solver's rrtLMC of every node in the context's own device array, the one
        node_cost_set writes and extend_select / find_new_target read with lmc=None.  cap: room offered to the first
        attempt; the buffers grow and the call is made once more when more nodes changed."""
        if cap is None:
            cap = 4096
        passes = C.c_int32()

        def call(cap, needed):
            node = np.empty(max(cap, 1), dtype=np.int32)
            lmc = np.empty(max(cap, 1), dtype=np.float64)
            par = np.empty(max(cap, 1), dtype=np.int32)
            return self._lib.rrtx_graph_cost_update_delta(self._h, int(root_idx), 1 if store else 0, _capi._ptr(node),
                                                          _capi._ptr(lmc), _capi._ptr(par), cap, needed,
                                                          C.byref(passes)), (node, lmc, par)
        n, (node, lmc, par) = self._two_call(cap, call)
        return node[:n], lmc[:n], par[:n], passes.value

    def graph_cost_to_root_dev(self, root_idx: int, lmc_ptr: int, parent_edge_ptr: Optional[int] = None):
        """rrtx_graph_cost_to_root_dev: rrtLMC (n_nodes doubles) and parent edges (n_nodes int32, or None) into device
        buffers, on the context's stream"""
        self._check(self._lib.rrtx_graph_cost_to_root_dev(self._h, int(root_idx), lmc_ptr, parent_edge_ptr))

    def graph_cost_update_dev(self, root_idx: int, lmc_ptr: int, parent_edge_ptr: Optional[int] = None):
        """rrtx_graph_cost_update_dev: graph_cost_to_root_dev continuing from the previous solve"""
        self._check(self._lib.rrtx_graph_cost_update_dev(self._h, int(root_idx), lmc_ptr, parent_edge_ptr))

    def obstacle_sweep(self, obstacle: int, search_range: float, robot_radius: float, cap: Optional[int] = None):
        """addNewObstacle's edge loop: ids (ascending) of the registered edges that start within
        search_range of sphere `obstacle` and collide with it."""
        if cap is None:
            cap = 4096

        def call(cap, needed):
            ids = np.empty(max(cap, 1), dtype=np.int32)
            return self._lib.rrtx_obstacle_sweep(self._h, obstacle, search_range, robot_radius, _capi._ptr(ids), cap,
                                                 needed), ids
        n, ids = self._two_call(cap, call)
        return ids[:n]

    def obstacle_sweep_batch(self, obstacles, search_range, robot_radius: float, block: bool = False,
                             cap: Optional[int] = None):
        """obstacle_sweep for a burst of sphere obstacles in one pass over the mirror (rrtx_obstacle_sweep_batch):
        returns (offsets, edge_ids), row j = edge_ids[offsets[j]:offsets[j + 1]] being exactly
        obstacle_sweep(obstacles[j], search_range[j], robot_radius); rows in the order given.  search_range: one range
        per obstacle (a scalar serves all).  block=True also blocks every returned edge in the mirror, on the device
        (what graph_edges_block over the union of the rows does)."""
        return self._sphere_burst(self._lib.rrtx_obstacle_sweep_batch, obstacles, search_range, robot_radius, block, cap)

    def obstacle_release_batch(self, obstacles, search_range, robot_radius: float, unblock: bool = False,
                               cap: Optional[int] = None):
        """The edge loops of a burst of corrected removeObstacle calls in one pass over the mirror
        (rrtx_obstacle_release_batch): returns (offsets, edge_ids), row j = the blocked edges that start within
        search_range[j] of sphere obstacles[j], collide with it (its own flag is not read) and with no sphere that is
        in use and not among `obstacles`; rows in the order given.  search_range: one range per obstacle (a scalar
        serves all).  unblock=True also gives every returned edge its original cost back in the mirror, on the device
        (what graph_edges_unblock over the union of the rows does)."""
        return self._sphere_burst(self._lib.rrtx_obstacle_release_batch, obstacles, search_range, robot_radius, unblock, cap)

    def _sphere_burst(self, fn, obstacles, search_range, robot_radius, apply, cap):
        obs = np.ascontiguousarray(obstacles, dtype=np.int32).reshape(-1)
        k = obs.shape[0]
        rng = np.ascontiguousarray(np.broadcast_to(np.asarray(search_range, dtype=np.float64), (k,)))
        if cap is None:
            cap = 4096

        def call(cap, needed):
            off = np.zeros(k + 1, dtype=np.int64)
            ids = np.empty(max(cap, 1), dtype=np.int32)
            return fn(self._h, _capi._ptr(obs), k, _capi._ptr(rng), robot_radius, 1 if apply else 0, _capi._ptr(off),
                      _capi._ptr(ids), cap, needed), (off, ids)
        n, (off, ids) = self._two_call(cap, call)
        return off, ids[:n]

    def obstacle_sweep_polygon(self, obstacle: int, robot_radius: float, delta: float, r_min: float = 0.0,
                               remove: bool = False, cap: Optional[int] = None):
        """The edge loops of addNewObstacle / removeObstacle for the polygon list (R/DRRT.jl:3048-3290): ids
        (ascending) of the mirrored edges that start at a node in conflict with polygon `obstacle` and collide with it
        (remove: that are blocked, collide with it and with no other obstacle in use).  SimpleEdge in a dim = 3
        context, DubinsEdge (r_min) in a dim = 4 one."""
        if cap is None:
            cap = 4096

        def call(cap, needed):
            ids = np.empty(max(cap, 1), dtype=np.int32)
            return self._lib.rrtx_obstacle_sweep_polygon(self._h, obstacle, robot_radius, delta, r_min, 1 if remove else 0,
                                                         _capi._ptr(ids), cap, needed), ids
        n, ids = self._two_call(cap, call)
        return ids[:n]

    def obstacle_sweep_polygon_batch(self, obstacles, robot_radius: float, delta: float, r_min: float = 0.0,
                                     block: bool = False, cap: Optional[int] = None):
        """obstacle_sweep_polygon (addNewObstacle's loop, remove=False) for a burst of polygon list positions in one
        call (rrtx_obstacle_sweep_polygon_batch): returns (offsets, edge_ids), row j =
        edge_ids[offsets[j]:offsets[j + 1]] being exactly obstacle_sweep_polygon(obstacles[j], robot_radius, delta,
        r_min); rows in the order given.  block=True also blocks every returned edge in the mirror, on the device (what
        graph_edges_block over the union of the rows does)."""
        return self._polygon_burst(self._lib.rrtx_obstacle_sweep_polygon_batch, obstacles, robot_radius, delta, r_min, block, cap)

    def obstacle_release_polygon_batch(self, obstacles, robot_radius: float, delta: float, r_min: float = 0.0,
                                       unblock: bool = False, cap: Optional[int] = None):
        """The edge loops of a burst of removeObstacle calls for the polygon list in one call
        (rrtx_obstacle_release_polygon_batch): returns (offsets, edge_ids), row j = the blocked edges that start at a
        node in conflict with polygon obstacles[j], collide with it (it must be in use: its flag is read) and with no
        polygon that is in use and not among `obstacles` -- obstacle_sweep_polygon(obstacles[j], ..., remove=True) with
        the other listed positions switched off; rows in the order given.  unblock=True also gives every returned edge
        its original cost back in the mirror, on the device (what graph_edges_unblock over the union of the rows does).
        Clear the flags afterwards with polygons_set_active."""
        return self._polygon_burst(self._lib.rrtx_obstacle_release_polygon_batch, obstacles, robot_radius, delta, r_min, unblock, cap)

    def _polygon_burst(self, fn, obstacles, robot_radius, delta, r_min, apply, cap):
        obs = np.ascontiguousarray(obstacles, dtype=np.int32).reshape(-1)
        k = obs.shape[0]
        if cap is None:
            cap = 4096

        def call(cap, needed):
            off = np.zeros(k + 1, dtype=np.int64)
            ids = np.empty(max(cap, 1), dtype=np.int32)
            return fn(self._h, _capi._ptr(obs), k, robot_radius, delta, r_min, 1 if apply else 0, _capi._ptr(off),
                      _capi._ptr(ids), cap, needed), (off, ids)
        n, (off, ids) = self._two_call(cap, call)
        return off, ids[:n]

    def polygons_set_active(self, obstacles, active):
        """The in-use flag of polygon list positions (rrtx_polygons_set_active): shapes and paths stay.  active: one
        value per position (a scalar serves all)."""
        obs = np.ascontiguousarray(obstacles, dtype=np.int32).reshape(-1)
        k = obs.shape[0]
        act = np.ascontiguousarray(np.broadcast_to(np.asarray(active).astype(bool).astype(np.uint8), (k,)))
        self._check(self._lib.rrtx_polygons_set_active(self._h, _capi._ptr(obs), k, _capi._ptr(act)))

    def dubins_edges_check_obstacle(self, s, g, r_min: float, robot_radius: float, obstacle: int):
        """explicitEdgeCheck(S, edge::DubinsEdge, ob) against polygon `obstacle` alone."""
        s = f64(s, (-1, 4))
        g = f64(g, (-1, 4))
        hit = np.empty(s.shape[0], dtype=np.uint8)
        self._check(self._lib.rrtx_dubins_edges_check_obstacle(self._h, _capi._ptr(s), _capi._ptr(g), s.shape[0], r_min,
                                                               robot_radius, obstacle, _capi._ptr(hit)))
        return hit

    def edges_check_idx(self, start_idx, end_idx, robot_radius: float, obstacle: int = -1, obstacle_mask=None,
                        want_first: bool = True):
        """Edges as node-index pairs (obstacle sweeps, R/DRRT_Q.jl:3220-3362)."""
        s = np.ascontiguousarray(start_idx, dtype=np.int32)
        e = np.ascontiguousarray(end_idx, dtype=np.int32)
        ne = s.shape[0]
        hit = np.empty(ne, dtype=np.uint8)
        first = np.empty(ne, dtype=np.int32) if want_first else None
        mask = None if obstacle_mask is None else np.ascontiguousarray(obstacle_mask, dtype=np.uint8)
        self._check(self._lib.rrtx_edges_check_idx(self._h, _capi._ptr(s), _capi._ptr(e), ne, robot_radius, obstacle,
                                                   _capi._ptr(mask), _capi._ptr(hit), _capi._ptr(first)))
        return hit, first
