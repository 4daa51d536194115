"""Obstacles that move in time (kinds 6 / 7) on lattices in time: a numpy restatement of findIndexBeforeTime,
findTransformObsToTimeOfPoint and the moving branch of explicitEdgeCheck2D (R/DRRT_Q.jl:1351-1391, 1699-1771; DESIGN.md
4.6), and the scenes tests/test_moving_lattice_scenes.py judges and tests/test_gpu_moving_lattice.py runs on the device.

Every coordinate, path offset and radius is a multiple of 1/4; every duration, of an edge and of a path segment, is a
power of two between 1/4 and 8 (or zero where a NaN is the subject).  The slopes of the rule are then exact, and so is
every product and sum up to num and den; T_c = num / den is exact wherever a scene places a closest approach on a
lattice time, which is where the ties are.  Polygons are diamonds (+-r, 0), (0, +-r) about a lattice centre: the
constructor's bounding radius is exactly r.

segment_tests() returns, per (edge, path segment), whether the rule tests the pair, the clamp state of T_c, T_c and
d^2 - rr^2; the rule's answer is any(d^2 - rr^2 < 0).  le_index / le_final restate the rule with `<=` in
findIndexBeforeTime / in the final comparison: a scene that is to notice such a mistake must hold edges on which the
answer changes, and the scene tests count them.

Static polygons (kind 3, in `crowd`) are not this model's subject: their per-obstacle answers are taken from the
oracle (static_hits), which tests/test_oracle_kat.py pins."""
import math

import numpy as np

Q = 0.25
LO, IN, HI, NAN = 0, 1, 2, 3


class Scene:
    """polys / kinds / active / paths in list order, directed edges p0 -> p1 as rows of (x, y, t), one robot radius,
    and tags: name -> index array of the edges built for that purpose."""

    def __init__(self, name, robot_radius):
        self.name, self.robot_radius = name, float(robot_radius)
        self.polys, self.kinds, self.active, self.paths, self.centres, self.radii = [], [], [], [], [], []
        self._p0, self._p1, self._tags = [], [], {}
        self.points = np.zeros((0, 3))

    def add_obstacle(self, cx, cy, r, kind, path=None, active=1):
        for v in (cx, cy, r):
            assert v * 4 == round(v * 4), "off the lattice"
        self.polys.append(diamond(cx, cy, r))
        self.kinds.append(kind)
        self.active.append(active)
        self.paths.append(None if path is None else np.asarray(path, dtype=np.float64).reshape(-1, 3))
        self.centres.append((float(cx), float(cy)))
        self.radii.append(float(r))
        return len(self.polys) - 1

    def add_edge(self, a, b, tag=None, flip=False):
        a, b = (b, a) if flip else (a, b)
        self._p0.append(tuple(float(v) for v in a))
        self._p1.append(tuple(float(v) for v in b))
        if tag is not None:
            self._tags.setdefault(tag, []).append(len(self._p0) - 1)
        return len(self._p0) - 1

    def finish(self):
        self.p0 = np.array(self._p0, dtype=np.float64).reshape(-1, 3)
        self.p1 = np.array(self._p1, dtype=np.float64).reshape(-1, 3)
        self.tags = {k: np.array(v, dtype=np.int64) for k, v in self._tags.items()}
        self.active = np.array(self.active, dtype=np.uint8)
        self.m = len(self.polys)
        self.moving = [j for j in range(self.m) if self.kinds[j] in (6, 7)]
        on_lattice(self)
        return self

    def polygon_set(self, oracle):
        ps = oracle.PolygonSet(self.polys, kinds=self.kinds, active=self.active, paths=self.paths)
        cr = ps.centre_radius()
        want = np.c_[np.array(self.centres).reshape(-1, 2), np.array(self.radii)]
        assert np.array_equal(cr, want), "the constructor's centre / bounding radius is not the diamond's"
        return ps


def diamond(cx, cy, r):
    return np.array([[cx + r, cy], [cx, cy + r], [cx - r, cy], [cx, cy - r]], dtype=np.float64)


def _pow2_or_zero(d):
    d = np.abs(np.asarray(d, dtype=np.float64)).ravel()
    d = d[d != 0]
    return bool(np.all((d >= 0.25) & (d <= 8.0) & (np.log2(d) == np.rint(np.log2(d)))))


def on_lattice(s):
    """the lattice contract of a finished scene"""
    for a in (s.p0, s.p1, s.points):
        assert np.array_equal(a * 4, np.rint(a * 4)), "an edge or point off the lattice"
    assert _pow2_or_zero(s.p1[:, 2] - s.p0[:, 2]), "an edge duration that is no power of two in [1/4, 8]"
    assert len(s.p0) <= 4096
    for p in s.paths:
        if p is not None:
            assert 1 <= len(p) <= 8 and np.array_equal(p * 4, np.rint(p * 4)), "a path off the lattice"
            assert _pow2_or_zero(np.diff(p[:, 2])) and np.all(np.diff(p[:, 2]) >= 0)


# ---- the rule ---------------------------------------------------------------------------------------------------------
def index_before_time(path_t, t, le=False):
    """findIndexBeforeTime for an array of times: the number of leading rows with time < t (le: <=, the mistake)"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    before = (path_t[None, :] <= t) if le else (path_t[None, :] < t)
    return np.logical_and.accumulate(before, axis=1).sum(axis=1)


def transform_obs_to_time(path, t, le=False):
    """findTransformObsToTimeOfPoint: the offset (dx, dy) of the obstacle at the times t"""
    t = np.asarray(t, dtype=np.float64).ravel()
    n = len(path)
    before = index_before_time(path[:, 2], t, le)
    b = path[np.clip(before - 1, 0, n - 1)]
    a = path[np.clip(before, 0, n - 1)]
    with np.errstate(all="ignore"):
        along = (t - b[:, 2]) / (a[:, 2] - b[:, 2])
        dx = b[:, 0] + along * (a[:, 0] - b[:, 0])
        dy = b[:, 1] + along * (a[:, 1] - b[:, 1])
    first, last = before < 1, before == n
    dx = np.where(first, path[0, 0], np.where(last, path[n - 1, 0], dx))
    dy = np.where(first, path[0, 1], np.where(last, path[n - 1, 1], dy))
    return dx, dy


def segment_tests(cx, cy, radius, path, p0, p1, robot_radius, le_index=False):
    """The moving branch of explicitEdgeCheck2D for one obstacle and the edges p0 -> p1: dict of [E, S] arrays (S =
    path rows - 1) `tested`, `state` (LO / IN / HI / NAN), `T_c` (after the clamp) and `margin` = d^2 - rr^2, plus
    `first` / `last` per edge.  A column is path segment is -> is + 1 (1-based is = column + 1)."""
    E = len(p0)
    n = 0 if path is None else len(path)
    S = max(n - 1, 0)
    out = dict(tested=np.zeros((E, S), dtype=bool), state=np.full((E, S), NAN, dtype=np.int8),
               T_c=np.full((E, S), np.nan), margin=np.full((E, S), np.nan),
               first=np.zeros(E, dtype=np.int64), last=np.zeros(E, dtype=np.int64))
    if n < 1:
        return out
    fwd = p0[:, 2] < p1[:, 2]
    early = np.where(fwd[:, None], p0, p1)
    late = np.where(fwd[:, None], p1, p0)
    first = np.maximum(index_before_time(path[:, 2], early[:, 2], le_index), 1)
    last = np.minimum(1 + index_before_time(path[:, 2], late[:, 2], le_index), n)
    out["first"], out["last"] = first, last
    rr = radius + robot_radius
    with np.errstate(all="ignore"):
        for c in range(S):
            is_ = c + 1
            pa, pb = path[is_ - 1], path[is_]
            x_1, y_1, T_1 = early[:, 0], early[:, 1], early[:, 2]
            x_2, y_2, T_2 = pa[0] + cx, pa[1] + cy, pa[2]
            m_x1 = (late[:, 0] - x_1) / (late[:, 2] - T_1)
            m_y1 = (late[:, 1] - y_1) / (late[:, 2] - T_1)
            m_x2 = np.float64((pb[0] + cx) - x_2) / np.float64(pb[2] - T_2)
            m_y2 = np.float64((pb[1] + cy) - y_2) / np.float64(pb[2] - T_2)
            num = (((m_x1 * m_x1) * T_1 + m_x2 * (((m_x2 * T_2) + x_1) - x_2)) -
                   m_x1 * (((m_x2 * (T_1 + T_2)) + x_1) - x_2)) + (m_y1 - m_y2) * ((((m_y1 * T_1) - (m_y2 * T_2)) - y_1) + y_2)
            den = (m_x1 - m_x2) * (m_x1 - m_x2) + (m_y1 - m_y2) * (m_y1 - m_y2)
            T_c = num / den
            lo_c = np.maximum(T_1, T_2)
            hi_c = np.minimum(late[:, 2], pb[2])
            is_lo = T_c < lo_c
            is_hi = ~is_lo & (T_c > hi_c)
            state = np.where(is_lo, LO, np.where(is_hi, HI, np.where(np.isnan(T_c), NAN, IN))).astype(np.int8)
            T_c = np.where(is_lo, lo_c, np.where(is_hi, hi_c, T_c))
            r_x = m_x1 * (T_c - T_1) + x_1
            r_y = m_y1 * (T_c - T_1) + y_1
            o_x = m_x2 * (T_c - T_2) + x_2
            o_y = m_y2 * (T_c - T_2) + y_2
            d2 = (r_x - o_x) * (r_x - o_x) + (r_y - o_y) * (r_y - o_y)
            tested = (first <= is_) & (is_ <= last - 1)
            out["tested"][:, c] = tested
            out["state"][:, c] = np.where(np.isnan(d2), NAN, state)
            out["T_c"][:, c] = T_c
            out["margin"][:, c] = d2 - rr * rr
    return out


def obstacle_hits(s, j, le_index=False, le_final=False, p0=None, p1=None, robot_radius=None):
    """the rule's answer for moving obstacle j of the scene, per edge (the active flag is not read)"""
    p0 = s.p0 if p0 is None else p0
    p1 = s.p1 if p1 is None else p1
    rr = s.robot_radius if robot_radius is None else robot_radius
    t = segment_tests(s.centres[j][0], s.centres[j][1], s.radii[j], s.paths[j], p0, p1, rr, le_index)
    with np.errstate(invalid="ignore"):
        below = (t["margin"] <= 0) if le_final else (t["margin"] < 0)
    return (t["tested"] & below).any(axis=1)


def static_hits(oracle, s, ps=None):
    """[m, E] bool: the oracle's explicitEdgeCheck2D of every edge against each kind 3 obstacle alone (flag not read)"""
    out = np.zeros((s.m, len(s.p0)), dtype=bool)
    for j in range(s.m):
        if s.kinds[j] == 3:
            one = oracle.PolygonSet([s.polys[j]])
            out[j] = oracle.edges_check_batch(one, s.p0, s.p1, s.robot_radius)[0].astype(bool)
    return out


def list_check(s, stat=None, le_index=False, le_final=False, only=None):
    """explicitEdgeCheck over the list: (hit, first-hit index) from the model's moving answers and `stat` for kind 3"""
    E = len(s.p0)
    hit = np.zeros(E, dtype=np.uint8)
    first = np.full(E, -1, dtype=np.int32)
    for j in range(s.m - 1, -1, -1):
        if not s.active[j] or (only is not None and j not in only):
            continue
        h = obstacle_hits(s, j, le_index, le_final) if s.kinds[j] in (6, 7) else stat[j]
        hit[h] = 1
        first[h] = j
    return hit, first


def count_states(s, tag=None):
    """per clamp state: (segment tests, exact ties d^2 == rr^2) over the scene's moving obstacles"""
    sel = slice(None) if tag is None else s.tags[tag]
    tests, ties = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for j in s.moving:
        if not s.active[j]:
            continue
        t = segment_tests(s.centres[j][0], s.centres[j][1], s.radii[j], s.paths[j], s.p0[sel], s.p1[sel], s.robot_radius)
        for k in range(4):
            m = t["tested"] & (t["state"] == k)
            tests[k] += m.sum()
            ties[k] += (m & (t["margin"] == 0)).sum()
    return tests, ties


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _path(t0, durs, start, steps):
    """rows (dx, dy, t): from offset `start` at time t0, segment k lasts durs[k] and moves by steps[k]"""
    rows = [(start[0], start[1], t0)]
    for d, (ax, ay) in zip(durs, steps):
        x, y, t = rows[-1]
        rows.append((x + ax, y + ay, t + d))
    return np.array(rows, dtype=np.float64)


def _pos(s, j, k):
    """where path row k (0-based) of obstacle j puts its centre, and when"""
    p = s.paths[j][k]
    return s.centres[j][0] + p[0], s.centres[j][1] + p[1], p[2]


NEAR = [(0.0, 0.0), (0.25, 0.0), (0.0, -0.5), (0.75, 1.0), (-1.0, 0.75), (1.25, 0.0), (0.0, 1.25), (-1.5, 0.0),
        (1.0, 1.0), (-0.75, -1.0), (1.5, 0.25), (0.0, -1.75), (2.0, 0.0)]


def knots():
    """Edges whose start or end time, or both, is a row time.  Robot radius 1/2, obstacle radius 3/4: rr = 5/4, and the
    offsets of NEAR lie inside it, on it ((3/4, 1), (5/4, 0)) and outside.  The robot's other end is far away (it
    moves at 8 or more per unit of time, away from the path), so that what happens AT the row time decides:
      - a start on the LAST row's time tests the last segment at that instant alone (`<`: the row is not before the
        time); a quarter later the edge lies after the path and nothing is tested;
      - an end on the FIRST row's time lies wholly before the path (`last` = 1): no test, although the robot may end on
        top of the obstacle; a quarter later the first segment is tested;
      - inner rows: both adjoining segments see the same instant, the answer cannot depend on which is tested."""
    s = Scene("knots", 0.5)
    rng = np.random.default_rng(61)
    for j in range(6):
        n = (4, 5, 6, 8, 4, 3)[j]
        durs = [float(2.0 ** rng.integers(0, 3)) for _ in range(n - 1)]
        steps = [(float(rng.integers(-8, 9)) * Q * 2, float(rng.integers(-8, 9)) * Q * 2) for _ in range(n - 1)]
        s.add_obstacle(48.0 * j, 8.0 * (j % 2), 0.75, 6 if j % 2 else 7,
                       _path(4.0 + j, durs, (float(rng.integers(-4, 5)), float(rng.integers(-4, 5))), steps))
    far = [(24.0, 16.0), (-16.0, 24.0), (-24.0, -16.0), (16.0, -24.0)]
    for j in range(6):
        n = len(s.paths[j])
        for row, tag in ((0, "first"), (n // 2, "inner"), (n - 1, "last")):
            x, y, t = _pos(s, j, row)
            for oi, (ox, oy) in enumerate(NEAR):
                for end in ("start", "end"):
                    for shift in (-Q, 0.0, Q):
                        for dur in (1.0, 2.0):
                            fx, fy = far[(oi + int(dur)) % 4]
                            here = (x + ox, y + oy, t + shift)
                            there = (x + ox + fx, y + oy + fy, t + shift + (dur if end == "start" else -dur))
                            a, b = (here, there) if end == "start" else (there, here)
                            s.add_edge(a, b, tag if shift == 0.0 else None, flip=(oi + row) % 2 == 1)
        # both ends on row times: the edge spans exactly one segment
        for row in range(n - 1):
            x, y, t = _pos(s, j, row)
            x2, y2, t2 = _pos(s, j, row + 1)
            for oi, (ox, oy) in enumerate(NEAR[:8]):
                tag = "first" if row == 0 else ("last" if row + 1 == n - 1 else "inner")
                s.add_edge((x + ox, y + oy, t), (x2 + 8.0, y2 - 6.0, t2), tag, flip=oi % 2 == 1)
        # wholly before the path and wholly after it, resting on top of where the obstacle starts / ends
        x, y, t = _pos(s, j, 0)
        x2, y2, t2 = _pos(s, j, n - 1)
        for oi, (ox, oy) in enumerate(NEAR[:6]):
            s.add_edge((x + ox, y + oy, t - 2.0 - Q * oi), (x + ox + Q, y + oy, t - 1.0 - Q * oi), "before", flip=oi % 2 == 1)
            s.add_edge((x2 + ox, y2 + oy, t2 + Q + Q * oi), (x2 + ox + Q, y2 + oy, t2 + 0.5 + Q + Q * oi), "after", flip=oi % 2 == 1)
    return s.finish()


# offsets of exact length: (dx, dy, |d|)
_TRIPLES = [(2.0, 0.0, 2.0), (0.0, 2.0, 2.0), (-2.0, 0.0, 2.0), (0.0, -2.0, 2.0),
            (0.75, 1.0, 1.25), (-1.0, 0.75, 1.25), (-0.75, -1.0, 1.25), (1.0, -0.75, 1.25),
            (1.5, 2.0, 2.5), (-2.0, -1.5, 2.5), (1.25, 3.0, 3.25), (-3.0, 1.25, 3.25), (3.0, -1.25, 3.25), (-1.25, -3.0, 3.25)]
_RR = (1.25, 2.0, 2.5, 3.25)


def tangent(robot_radius):
    """Closest approach exactly at rr^2 in each clamp state, and one lattice step to every side of it.  Obstacle k has
    radius _RR[k] - robot_radius and moves at integer velocity u on segments of 4 or 8; T* is a lattice time strictly
    inside a segment, O* the obstacle's centre then, d an offset of exact length rr, w the relative velocity:
      in   w perpendicular to d, the edge spans T* -+ D/2 (also with T* ON the edge's start or end: T_c lands exactly on
           a clamp and is still `in`)
      lo   the edge starts at T* in O* + d and w . d > 0: the closest approach is past, T_c is clamped to the start
      hi   the edge ends at T* in O* + d and w . d < 0."""
    s = Scene("tangent_%g" % robot_radius, robot_radius)
    us = [(1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (-2.0, 1.0)]
    for k, R in enumerate(_RR):
        durs = [4.0, 8.0, 4.0]
        steps = [(us[(k + i) % 4][0] * d, us[(k + i) % 4][1] * d) for i, d in enumerate(durs)]
        s.add_obstacle(64.0 * k, 0.0, R - robot_radius, 6 if k % 2 else 7, _path(2.0, durs, (-4.0, 3.0), steps))
    shifts = [(0.0, 0.0), (Q, 0.0), (-Q, 0.0), (0.0, Q), (0.0, -Q)]
    n = 0
    for k, R in enumerate(_RR):
        for (dx, dy, L) in _TRIPLES:
            if L != R:
                continue
            for seg in range(3):
                x0, y0, t0 = _pos(s, k, seg)
                x1, y1, t1 = _pos(s, k, seg + 1)
                u = ((x1 - x0) / (t1 - t0), (y1 - y0) / (t1 - t0))
                for lam in (1.0, -2.0):
                    n += 1
                    Ts = t0 + 1.25 + Q * (n % 4)                      # strictly inside the segment, every edge below too
                    ox, oy = x0 + u[0] * (Ts - t0), y0 + u[1] * (Ts - t0)
                    f = {1.25: 4.0, 2.5: 2.0, 3.25: 4.0, 2.0: 0.5}[L]
                    wd = (dx * f, dy * f)                              # integer vector along d: (3, 4), (5, 12), (1, 0) ...
                    wp = (-dy * f, dx * f)                             # ... and across it
                    for state in ("in", "in_lo", "in_hi", "lo", "hi"):
                        D = (0.5, 1.0, 2.0)[n % 3] if state == "in" else (0.25, 0.5, 1.0)[n % 3]
                        if state.startswith("in"):
                            v = (u[0] + lam * wp[0], u[1] + lam * wp[1])
                            before = {"in": D / 2, "in_lo": 0.0, "in_hi": D}[state]
                        else:
                            sign = abs(lam) if state == "lo" else -abs(lam)
                            v = (u[0] + sign * wd[0] + lam * wp[0] * (n % 2), u[1] + sign * wd[1] + lam * wp[1] * (n % 2))
                            before = 0.0 if state == "lo" else D
                        for (hx, hy) in shifts:
                            a = (ox + dx - v[0] * before + hx, oy + dy - v[1] * before + hy, Ts - before)
                            b = (a[0] + v[0] * D, a[1] + v[1] * D, a[2] + D)
                            s.add_edge(a, b, state if (hx, hy) == (0.0, 0.0) else "near_" + state, flip=n % 2 == 1)
    return s.finish()


def nan_scene():
    """The quotients that go NaN and mean "no hit", each with the robot overlapping the obstacle:
      same_velocity  robot and obstacle move alike (den == 0, num == 0)
      zero_duration  edges with t0 == t1 (slopes +-Inf or 0/0)
      zero_length    p0 == p1 entirely, and edges that rest in place against an obstacle that rests (den == 0)
      repeat_mid / repeat_end   a path with a repeated row time: the segment between the twin rows has no duration
      single_row     a one-row path is never tested."""
    s = Scene("nan", 0.5)
    j0 = s.add_obstacle(0.0, 0.0, 1.0, 6, _path(2.0, [4.0, 2.0, 4.0], (1.0, -1.0), [(4.0, 0.0), (0.0, 0.0), (-2.0, 4.0)]))
    j1 = s.add_obstacle(40.0, 0.0, 1.0, 7, _path(1.0, [2.0, 0.0, 2.0], (0.0, 0.0), [(2.0, 0.0), (6.0, 0.0), (0.0, 2.0)]))     # twin rows in the middle
    j2 = s.add_obstacle(80.0, 0.0, 1.0, 6, _path(1.0, [0.0, 4.0], (0.0, 0.0), [(5.0, 0.0), (0.0, 4.0)]))                       # twin rows at the start
    j3 = s.add_obstacle(120.0, 0.0, 1.0, 7, _path(1.0, [4.0, 0.0], (0.0, 0.0), [(0.0, 4.0), (5.0, 0.0)]))                      # twin rows at the end
    j4 = s.add_obstacle(160.0, 0.0, 1.0, 6, _path(3.0, [0.0], (0.0, 0.0), [(4.0, 0.0)]))                                       # two rows, one time
    j5 = s.add_obstacle(200.0, 0.0, 1.0, 7, np.array([[1.0, 1.0, 5.0]]))                                                        # a single row
    offs = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.75), (-1.0, 0.5), (0.75, 1.0), (1.25, 0.0), (0.0, 1.75), (2.0, 0.0)]
    for i, (ox, oy) in enumerate(offs):
        # same velocity, inside each segment that moves (0: u = (1, 0); 2: u = (-1/2, 1))
        for seg, dur in ((0, 2.0), (0, 1.0), (2, 2.0), (2, 1.0)):
            x0, y0, t0 = _pos(s, j0, seg)
            x1, y1, t1 = _pos(s, j0, seg + 1)
            u = ((x1 - x0) / (t1 - t0), (y1 - y0) / (t1 - t0))
            a = (x0 + u[0] * 0.5 + ox, y0 + u[1] * 0.5 + oy, t0 + 0.5)   # strictly inside the segment: it alone is tested
            s.add_edge(a, (a[0] + u[0] * dur, a[1] + u[1] * dur, a[2] + dur), "same_velocity", flip=i % 2 == 1)
        # resting robot against the resting segment 1 of obstacle 0 (rows 1 and 2 share the position)
        x0, y0, t0 = _pos(s, j0, 1)
        for dur in (0.25, 0.5, 1.0):
            s.add_edge((x0 + ox, y0 + oy, t0 + Q), (x0 + ox, y0 + oy, t0 + Q + dur), "zero_length", flip=i % 2 == 1)
        # resting robot against a segment that moves: an ordinary test (the obstacle runs over it or not)
        s.add_edge((x0 - 2.0 + ox, y0 + oy, t0 - 4.0), (x0 - 2.0 + ox, y0 + oy, t0), "rest_vs_moving", flip=i % 2 == 1)
        for k in range(4):
            x, y, t = _pos(s, j0, k)
            s.add_edge((x + ox, y + oy, t + Q * i), (x + ox, y + oy, t + Q * i), "zero_length")
            s.add_edge((x + ox, y + oy, t + Q * i), (x + ox + 2.0, y + oy - 1.0 * (i % 2), t + Q * i), "zero_duration", flip=i % 2 == 1)
            s.add_edge((x + ox, y + oy, t + Q * i), (x + ox, y + oy + 0.5, t + Q * i), "zero_duration", flip=i % 2 == 1)
        # twin rows: edges across the shared time, from on top of either twin, and ones that only touch it
        for (j, row, tag) in ((j1, 1, "repeat_mid"), (j2, 0, "repeat_end"), (j3, 1, "repeat_end"), (j4, 0, "repeat_end")):
            xa, ya, t = _pos(s, j, row)
            xb, yb, _ = _pos(s, j, row + 1)
            for (x, y) in ((xa, ya), (xb, yb), ((xa + xb) / 2, (ya + yb) / 2)):
                x = math.floor(x * 4) / 4
                s.add_edge((x + ox, y + oy, t - 0.5), (x + ox + 0.5, y + oy, t + 0.5), tag, flip=i % 2 == 1)
                s.add_edge((x + ox, y + oy, t - 1.0), (x + ox, y + oy + Q, t + 1.0), tag, flip=i % 2 == 0)
                s.add_edge((x + ox, y + oy, t), (x + ox + 0.5, y + oy, t + 0.5), tag + "_touch")
                s.add_edge((x + ox, y + oy, t - 0.5), (x + ox + 0.5, y + oy, t), tag + "_touch")
        x, y, t = _pos(s, j5, 0)
        for (ta, tb) in ((t - 1.0, t + 1.0), (t, t + 2.0), (t - 2.0, t), (t - 4.0, t + 4.0)):
            s.add_edge((x + ox, y + oy, ta), (x + ox + Q, y + oy, tb), "single_row", flip=i % 2 == 1)
    return s.finish()


def far_record(robot_radius=0.5):
    """Obstacles whose record centre lies 100 units or more from where the path carries them: the diamonds stand about
    (200 + 100 k, 300) and every path offset starts near (-200 - 100 k, -300), so the centres move through [-12, 12]^2
    where the edges are.  A screen built on the record centre drops every hit of this scene."""
    s = Scene("far_record", robot_radius)
    rng = np.random.default_rng(67)
    for k in range(8):
        cx, cy = 200.0 + 100.0 * k, 300.0
        n = 3 + k % 4
        durs = [float(2.0 ** rng.integers(0, 3)) for _ in range(n - 1)]
        steps = [(float(rng.integers(-12, 13)) * Q * 2, float(rng.integers(-12, 13)) * Q * 2) for _ in range(n - 1)]
        start = (-cx + float(rng.integers(-32, 33)) * Q, -cy + float(rng.integers(-32, 33)) * Q)
        s.add_obstacle(cx, cy, (1.0, 1.5, 2.0, 2.5)[k % 4], 6 if k % 2 else 7, _path(float(k % 3), durs, start, steps))
    _random_edges(s, rng, 1200, 12.0, 12.0, 16.0)
    return s.finish()


def _random_edges(s, rng, n, span, t_lo_hi, reach):
    for i in range(n):
        a = (float(rng.integers(-span * 4, span * 4 + 1)) * Q, float(rng.integers(-span * 4, span * 4 + 1)) * Q,
             float(rng.integers(0, t_lo_hi * 4 + 1)) * Q)
        dur = float(2.0 ** rng.integers(-2, 4))
        b = (a[0] + float(rng.integers(-reach, reach + 1)) * Q, a[1] + float(rng.integers(-reach, reach + 1)) * Q, a[2] + dur)
        s.add_edge(a, b, None, flip=i % 2 == 1)


CROWD_MOVING_AT = (31, 32, 63, 64, 127, 128, 255, 256)


def crowd(m_active, n_edges=1024, seed=71, static=True):
    """m_active + 2 obstacles (two are inactive) on a grid of pitch 6, kinds 3 / 6 / 7 mixed (static=False: 6 / 7 only),
    moving ones at every list position of CROWD_MOVING_AT the list has, at least five moving ones in the first 32
    positions, and short edges all over the grid."""
    s = Scene("crowd_%d" % m_active, 0.5)
    rng = np.random.default_rng(seed + m_active)
    m = m_active + 2
    side = int(math.ceil(math.sqrt(m)))
    inactive = (5, m - 6)
    for j in range(m):
        cx, cy = 6.0 * (j % side), 6.0 * (j // side)
        kind = (3, 6, 7)[j % 3] if static else (6, 7)[j % 2]
        if j in CROWD_MOVING_AT or j in inactive:
            kind = 6 if j % 2 else 7
        r = (0.75, 1.0, 1.25, 1.5)[j % 4]
        path = None
        if kind != 3:
            n = 1 + int(rng.integers(1, 5)) if j % 11 else 1
            durs = [float(2.0 ** rng.integers(0, 3)) for _ in range(n - 1)]
            steps = [(float(rng.integers(-8, 9)) * Q, float(rng.integers(-8, 9)) * Q) for _ in range(n - 1)]
            path = _path(float(rng.integers(0, 9)) * Q, durs, (float(rng.integers(-4, 5)) * Q, float(rng.integers(-4, 5)) * Q), steps)
        s.add_obstacle(cx, cy, r, kind, path, active=0 if j in inactive else 1)
    span = 6.0 * side
    for i in range(n_edges):
        a = (float(rng.integers(-8, span * 4)) * Q, float(rng.integers(-8, span * 4)) * Q, float(rng.integers(0, 33)) * Q)
        dur = float(2.0 ** rng.integers(-2, 3))
        b = (a[0] + float(rng.integers(-20, 21)) * Q, a[1] + float(rng.integers(-20, 21)) * Q, a[2] + dur)
        s.add_edge(a, b, None, flip=i % 2 == 1)
    return s.finish()


def lattice_random(n_edges=4000, n_obs=24, seed=73):
    """seeded lattice draws for breadth: n_obs moving diamonds in [-12, 12]^2, n_edges edges"""
    s = Scene("lattice_random", 0.5)
    rng = np.random.default_rng(seed)
    for k in range(n_obs):
        n = int(rng.integers(1, 9))
        durs = [float(2.0 ** rng.integers(-2, 4)) for _ in range(n - 1)]
        steps = [(float(rng.integers(-16, 17)) * Q, float(rng.integers(-16, 17)) * Q) for _ in range(n - 1)]
        s.add_obstacle(float(rng.integers(-48, 49)) * Q, float(rng.integers(-48, 49)) * Q, float(rng.integers(1, 9)) * Q,
                       6 if k % 2 else 7, _path(float(rng.integers(0, 17)) * Q, durs, (float(rng.integers(-8, 9)) * Q, float(rng.integers(-8, 9)) * Q), steps))
    _random_edges(s, rng, n_edges, 14.0, 20.0, 24.0)
    return s.finish()


SCENES = {
    "knots": knots, "tangent_0.25": lambda: tangent(0.25), "tangent_0.5": lambda: tangent(0.5), "tangent_1": lambda: tangent(1.0),
    "nan": nan_scene, "far_record": far_record, "crowd_33": lambda: crowd(33), "crowd_65": lambda: crowd(65),
    "crowd_257": lambda: crowd(257), "lattice_random": lattice_random,
}
_built = {}


def scene(name):
    """a scene by name, built once"""
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


# ---- points -----------------------------------------------------------------------------------------------------------
def scene_points(s, per_obstacle=True):
    """Points (x, y, t) for explicitPointCheck against the scene's list: for every moving obstacle and each of its
    rows, at the row's time, a quarter before and after it (before the first row and after the last included), at
    offsets from where the obstacle is THEN (by transform_obs_to_time) of: the centre, a vertex + (robot radius, 0) --
    clearance exactly 0, not unsafe: `thisDist < 0.0` is strict --, a quarter nearer (unsafe) and a quarter farther."""
    pts = []
    rr = s.robot_radius
    for j in s.moving:
        path, (cx, cy), r = s.paths[j], s.centres[j], s.radii[j]
        times = sorted({float(t + d) for t in path[:, 2] for d in (-Q, 0.0, Q)} | {float(path[0, 2] - 3.0), float(path[-1, 2] + 5.0)})
        dx, dy = transform_obs_to_time(path, np.array(times))
        for t, ax, ay in zip(times, dx, dy):
            ax, ay = math.floor(ax * 4) / 4, math.floor(ay * 4) / 4          # (inside a segment the offset may leave the lattice)
            for (ox, oy) in ((0.0, 0.0), (r + rr, 0.0), (r + rr - Q, 0.0), (r + rr + Q, 0.0), (0.0, -(r + rr)), (-(r + rr), Q)):
                pts.append((cx + ax + ox, cy + ay + oy, t))
    return np.array(pts, dtype=np.float64).reshape(-1, 3)


def points_expected(oracle, s, pts, robot_radius=None):
    """explicitPointCheck of pts against the list, by the model's offsets: every moving obstacle is replaced by a
    static diamond moved by transform_obs_to_time(path, t) and the oracle's STATIC branch judges it.  On the lattice the
    moved vertices and centre are the same doubles either way, so flag and clearance must equal the moving branch's."""
    rr = s.robot_radius if robot_radius is None else robot_radius
    offs = {j: transform_obs_to_time(s.paths[j], pts[:, 2]) for j in s.moving}
    unsafe = np.zeros(len(pts), dtype=np.uint8)
    clr = np.zeros(len(pts))
    for i, p in enumerate(pts):
        polys = [s.polys[j] + (offs[j][0][i], offs[j][1][i]) if j in offs else s.polys[j] for j in range(s.m)]
        u, c = oracle.point_check_polygons(oracle.PolygonSet(polys, active=s.active), p, rr)
        unsafe[i], clr[i] = u, c
    return unsafe, clr


# ---- Dubins edges in a space with time: [x y t theta] -----------------------------------------------------------------
R_MIN = 1.0


def dubins_edges(s, n=1500, seed=79):
    """the scene's first n edges as Dubins edges: start later than end (planning runs in reverse time; edges without
    duration are left out), headings multiples of 1/4 rad drawn by seed"""
    rng = np.random.default_rng(seed)
    keep = np.flatnonzero(s.p0[:, 2] != s.p1[:, 2])[:n]
    a, b = s.p0[keep], s.p1[keep]
    back = a[:, 2] > b[:, 2]
    S = np.where(back[:, None], a, b)
    G = np.where(back[:, None], b, a)
    th = rng.integers(0, 25, (len(keep), 2)) * Q
    return np.c_[S, th[:, 0]], np.c_[G, th[:, 1]]


_DIRS = ((1.0, 0.0, 0.0), (0.0, 1.0, math.pi / 2), (-1.0, 0.0, math.pi), (0.0, -1.0, 3 * math.pi / 2))


def _straight(gx, gy, gt, d, length, dur):
    """a straight Dubins edge that arrives in (gx, gy) at time gt, heading d = (ux, uy, theta), from `length` behind"""
    return (gx - d[0] * length, gy - d[1] * length, gt + dur, d[2]), (gx, gy, gt, d[2])


def dubins_ties(robot_radius=0.5, r_min=R_MIN):
    """Straight edges (both headings along the chord) end exactly in the end node g: the polyline's last row is g
    itself, and so is the chord's end.  Obstacle: radius 1, first path row at time g.t at distance D from g -- beyond
    the end or abreast of it --, moving farther away afterwards, so the closest approach is at g.t (T_c clamped `lo`):
    D = R2 = radius + robot_radius is an exact tie of stage 2 (no hit), a quarter nearer a hit; D = R1 = R2 + 2 r_min
    is an exact tie of the chord test of stage 1 (which a straight edge cannot turn into a hit: stage 2 is the same
    line, 2 r_min farther than it would have to be).  Returns (scene of obstacles, S, G, tag per edge)."""
    s = Scene("dubins_ties", robot_radius)
    rad = 1.0
    R2 = rad + robot_radius
    R1 = R2 + 2 * r_min
    S, G, tags = [], [], []
    c = 0
    for d in _DIRS:
        for place in ("end", "side"):
            n = (d[0], d[1]) if place == "end" else (-d[1], d[0])
            for name, D in (("tie2", R2), ("in2", R2 - Q), ("out2", R2 + Q), ("tie1", R1), ("in1", R1 - Q), ("out1", R1 + Q)):
                gx, gy, gt = 8.0 + 40.0 * (c % 8), 8.0 + 40.0 * (c // 8), 2.0 + Q * (c % 3)
                c += 1
                path = np.array([[n[0] * D, n[1] * D, gt], [n[0] * (D + 4.0) + d[0] * 2.0, n[1] * (D + 4.0) + d[1] * 2.0, gt + 4.0]])
                s.add_obstacle(gx, gy, rad, 6 if c % 2 else 7, path)
                for length, dur in ((4.0, 1.0), (6.0, 2.0), (3.0, 4.0)):
                    a, b = _straight(gx, gy, gt, d, length, dur)
                    S.append(a); G.append(b); tags.append(name)
    s.finish()
    return s, np.array(S), np.array(G), np.array(tags)


DELTAS = (-1e-6, -1e-10, 0.0, 1e-10, 1e-6)


def dubins_screen_cases(robot_radius=0.5, r_min=R_MIN):
    """The two screens that exist only for obstacles that move (kernels_dubins.hip, stages 1a and 2a) compare the box
    of the obstacle's path with the chord's box, widened by R1 = radius + robot_radius + 2 r_min, and with a piece's
    box, widened by R2 = radius + robot_radius.  Here the path box lies at a gap of R (1 + delta) from the box of a
    straight edge (chord and pieces share it), beyond its end or beside it, in x and in y, on both sides; at time g.t
    the obstacle is abreast of g, at that very distance, and leaves.  With R = R2 and delta < 0 the oracle reports a
    hit that a screen with too small a radius drops; delta > 0 is no hit whatever the screen does; with R = R1 no
    straight edge is hit (the pieces lie on the chord), those rows hold the screen to "keeps or drops, same answer".
    So these rows hold the SIZE of stage 2a's radius and the centre of both boxes; the size of stage 1a's radius
    shows only on curved edges: dubins_curved_cases().
    Returns (scene, S, G, radius name per edge, delta per edge)."""
    s = Scene("dubins_screens", robot_radius)
    rad = 1.5
    R2 = rad + robot_radius
    R1 = R2 + 2 * r_min
    S, G, which, delta = [], [], [], []
    c = 0
    for d in _DIRS:
        for place in ("end", "side"):
            n = (d[0], d[1]) if place == "end" else (-d[1], d[0])
            t = (-n[1], n[0])                                   # the obstacle slides along its box's near side
            for name, R in (("R2", R2), ("R1", R1)):
                for dl in DELTAS:
                    gx, gy, gt = 8.0 + 48.0 * (c % 10), 8.0 + 48.0 * (c // 10), 3.0
                    c += 1
                    gap = R * (1.0 + dl)
                    path = np.array([[n[0] * gap - t[0] * 0.5, n[1] * gap - t[1] * 0.5, gt - 1.0],
                                     [n[0] * gap + t[0] * 0.5, n[1] * gap + t[1] * 0.5, gt + 1.0]])
                    s.polys.append(diamond(gx, gy, rad)); s.kinds.append(6 if c % 2 else 7); s.active.append(1)
                    s.paths.append(path); s.centres.append((gx, gy)); s.radii.append(rad)
                    for length, dur in ((4.0, 1.0), (6.0, 2.0)):
                        a, b = _straight(gx, gy, gt, d, length, dur)
                        S.append(a); G.append(b); which.append(name); delta.append(dl)
    s.p0 = s.p1 = np.zeros((0, 3))
    s.active = np.array(s.active, dtype=np.uint8)
    s.m = len(s.polys)
    s.moving = list(range(s.m))
    return s, np.array(S), np.array(G), np.array(which), np.array(delta)


CURVED_GAPS = (3.0, 3.5, 3.75, 4.25)


def dubins_curved_cases(robot_radius=0.5, r_min=R_MIN):
    """Where the SIZE of stage 1a's radius decides: an edge whose start lies 1 ahead of its end with the same heading
    must loop (a full right turn, word rsr), and the loop carries the robot up to 2 r_min to the right of the chord's
    box.  An obstacle of radius 1.5 dwells beside the box at a gap of 3, 3.5, 3.75 (all above R2 = radius +
    robot_radius = 2, below R1 = R2 + 2 r_min = 4) or 4.25, to the right or to the left.  To the right at 3 and 3.5 the
    oracle reports a hit, which a stage 1a with less than 2 r_min in its radius drops; at 4.25 and on the left nothing
    is hit.  Returns (scene, S, G, side per edge (-1 right, 1 left), gap per edge)."""
    s = Scene("dubins_curved", robot_radius)
    S, G, sides, gaps = [], [], [], []
    c = 0
    for (ux, uy, th) in _DIRS:
        for side in (-1.0, 1.0):
            n = (-uy * side, ux * side)
            for gap in CURVED_GAPS:
                gx, gy = 8.0 + 32.0 * (c % 8), 8.0 + 32.0 * (c // 8)
                c += 1
                s.add_obstacle(gx, gy, 1.5, 6 if c % 2 else 7,
                               np.array([[n[0] * gap - ux * 0.5, n[1] * gap - uy * 0.5, 1.0], [n[0] * gap + ux * 1.5, n[1] * gap + uy * 1.5, 9.0]]))
                S.append((gx + ux, gy + uy, 10.0, th)); G.append((gx, gy, 2.0, th)); sides.append(side); gaps.append(gap)
    s.finish()
    return s, np.array(S), np.array(G), np.array(sides), np.array(gaps)


# ---- sweeps: findPointsInConflictWithObstacle's one query per path segment --------------------------------------------
SWEEP_RR, SWEEP_DELTA = 0.5, 2.0
# lattice vectors of the plane scene's ranges, by range
_SWEEP_VEC = {3.5: [(1.5, 3.0, 1.0)], 5.0: [(3.0, 4.0, 0.0), (0.0, -3.0, 4.0)], 6.5: [(2.5, 6.0, 0.0), (1.5, 2.0, 6.0)],
              7.0: [(2.0, 3.0, 6.0), (-6.0, 2.0, 3.0)], 8.0: []}                   # (no lattice vector off the axes has length 8)


def sweep_queries(path, cx, cy, base):
    """the reference's range queries for a moving obstacle: [((x, y, t), range)], one per path segment i -> i + 1 about
    its midpoint with range base + |segment| / 2; a one-row path gives one query at the row with range base"""
    out = []
    for i in range(len(path)):
        k = 0 if len(path) == 1 else i + 1
        mid = (path[i] + path[k]) / 2.0
        out.append(((cx + mid[0], cy + mid[1], mid[2]), base + math.sqrt(((path[i] - path[k]) ** 2).sum()) / 2.0))
        if k == len(path) - 1:
            break
    return out


def sweep_scene(dubins, seed=83, n_nodes=1100):
    """A lattice tree and four moving obstacles of radius 1 whose path segments (dx, dy, dt) are the integer triples with
    an exact root (1, 2, 2) -> 3, (2, 3, 6) -> 7, (1, 4, 8) -> 9 and (2, 4, 4) -> 6: with base = robot radius + delta +
    radius = 3.5 every range base + |segment| / 2 is a lattice number (5, 7, 8, 6.5) and every query a lattice point.
    (The ranges are this scene's subject; its durations are not all powers of two.)  Obstacle 0 has two rows (one query),
    obstacle 1 four, obstacle 2 three, obstacle 3 a single row (one query at the row, range base); obstacle 4 is static.

    Around EVERY query nodes are planted exactly at its range R, a quarter inside and a quarter outside, along +-x, +-y
    and +-t (and, in the plane, along lattice vectors of length R).  dubins: nodes are [x y t theta], the query gets
    theta = pi and R = range + pi as the library adds it up; the planted nodes have theta = pi, and an axis direction is
    used only where (q + R) - q == R in doubles, so that "at" is exactly at.  Every planted node owns an edge that ends
    where the obstacle is at the segment's first row, then: the edge is hit (but for the one-row path, which is never
    tested), it is a candidate exactly when its start is in conflict, and a range or query that is off shows at once --
    in the returned ids, or, for the one-row path, in the number of candidate edges.
    Node 0, the root, lies exactly at the range of obstacle 0's only query and is listed by `<=`; node 1, the same
    place, is not.  Edges 0 and 1 lead from them to a point of obstacle 0's path.
    Returns dict(pts, es, ee, scene, queries: {j: [(q, range)]}, planted: {j: [(node, 'at' / 'in' / 'out')]})."""
    s = Scene("sweep_dubins" if dubins else "sweep_plane", SWEEP_RR)
    rad = 1.0
    base = SWEEP_RR + SWEEP_DELTA + rad
    s.add_obstacle(-1.0, -2.0, rad, 6, np.array([[0.0, 0.0, 2.0], [2.0, 4.0, 6.0]]))
    s.add_obstacle(10.0, 0.0, rad, 7, np.array([[0.0, 0.0, 1.0], [1.0, 2.0, 3.0], [3.0, 5.0, 9.0], [4.0, 9.0, 17.0]]))
    s.add_obstacle(-12.0, 6.0, rad, 6, np.array([[0.0, -4.0, 4.0], [2.0, 0.0, 8.0], [1.0, -2.0, 10.0]]))
    s.add_obstacle(0.0, 14.0, rad, 7, np.array([[2.0, 1.0, 5.0]]))
    s.add_obstacle(4.0, -10.0, rad, 3, None)
    s.p0 = s.p1 = np.zeros((0, 3))
    s.active = np.array(s.active, dtype=np.uint8)
    s.m = len(s.polys)
    s.moving = [0, 1, 2, 3]
    rng = np.random.default_rng(seed)
    extra = math.pi if dubins else 0.0
    at_pi, at_0 = ((math.pi,), (0.0,)) if dubins else ((), ())
    queries = {j: sweep_queries(s.paths[j], s.centres[j][0], s.centres[j][1], base) for j in s.moving}
    q0, r0 = queries[0][0]
    root = (q0[0], q0[1] + (r0 + extra), q0[2]) + at_pi
    pts = [root, root, (-0.5, -1.0, 3.0) + at_0]             # the third: where obstacle 0 IS at time 3
    es, ee = [0, 1], [2, 2]
    planted = {j: [] for j in s.moving}
    for j in s.moving:
        for i, (q, r) in enumerate(queries[j]):
            R = r + extra
            row = s.paths[j][i]
            target = len(pts)
            pts.append((s.centres[j][0] + row[0], s.centres[j][1] + row[1], row[2]) + at_0)
            spots = []
            for a in range(3):
                for sign in (1.0, -1.0):
                    if abs((q[a] + sign * R) - q[a]) != R:
                        continue
                    for name, dist in (("at", R), ("in", R - Q), ("out", R + Q)):
                        p = list(q)
                        p[a] = q[a] + sign * dist
                        spots.append((name, tuple(p)))
            for v in ([] if dubins else _SWEEP_VEC[r]):
                assert v[0] * v[0] + v[1] * v[1] + v[2] * v[2] == r * r
                L = max(range(3), key=lambda a: abs(v[a]))
                for name, step in (("at", 0.0), ("in", -Q), ("out", Q)):
                    w = list(v)
                    w[L] += step if v[L] > 0 else -step
                    spots.append((name, (q[0] + w[0], q[1] + w[1], q[2] + w[2])))
            for name, p in spots:
                planted[j].append((len(pts), name))
                es.append(len(pts)); ee.append(target)
                pts.append(p + at_pi)
    n_rand = n_nodes - len(pts)
    rnd = np.c_[rng.integers(-64, 81, n_rand) * Q, rng.integers(-56, 73, n_rand) * Q, rng.integers(0, 73, n_rand) * Q]
    if dubins:
        rnd = np.c_[rnd, rng.integers(0, 25, n_rand) * Q]
    pts = np.array(pts + [tuple(p) for p in rnd], dtype=np.float64).reshape(-1, 4 if dubins else 3)
    # the rest of the mirror: four out-edges per node to nodes nearby, earlier in time (planning runs in reverse time)
    for i in range(len(pts)):
        dd = np.abs(pts[:, :2] - pts[i, :2]).max(axis=1)
        cand = np.flatnonzero((dd <= 5.0) & (pts[:, 2] < pts[i, 2]) & (pts[i, 2] - pts[:, 2] <= 4.0))
        for k in rng.choice(cand, min(4, len(cand)), replace=False):
            es.append(i); ee.append(int(k))
    return dict(pts=pts, es=np.array(es, dtype=np.int32), ee=np.array(ee, dtype=np.int32), scene=s, planted=planted,
                queries=queries)


def sweep_listed(sc, j, dubins):
    """which planted nodes of obstacle j the rule lists: within (`<`) the range of ANY of j's queries (a node planted
    for one segment may lie inside the next one's ball).  {node: bool}; theta is pi on both sides, no ghost is nearer."""
    pts, extra = sc["pts"], (math.pi if dubins else 0.0)
    out = {}
    for node, _ in sc["planted"][j]:
        out[node] = any(math.sqrt(sum((pts[node][a] - q[a]) ** 2 for a in range(3))) < r + extra for q, r in sc["queries"][j])
    return out
