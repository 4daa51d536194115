"""Generator of tests/golden/time_column_flips.json: (Dubins edge, moving obstacle) cases on which the reference's
running-sum time column and the kernels' piecewise one give DIFFERENT collision booleans.  CPU only, oracle only:

    python tests/make_time_column_flips.py

The two columns differ in the last bits of the stamps of deep interior rows of a long arc.  A moving obstacle (kind 6,
bounding circle only, R/DRRT.jl:1579-1651) is tested against a piece at the time of closest approach of the two centres,
and that time is worked out from the piece's two stamps.  So a small obstacle that drifts slowly (0.02 per unit of time)
along the normal of ONE piece and grazes it from the inside of the arc -- its centre at robotRadius + radius from the
piece's chord, the neighbouring chords of the inscribed polygon 0.0075 r_min farther away -- collides or not on the last
bits of a squared distance.  For such a piece the obstacle's x offset is bisected to the double where the boolean of
that piece flips under the running sum, and the 97 doubles around it are scanned for one where the two columns
disagree; a case is kept when the WHOLE edge check (both stages, every piece) disagrees too.  Everything in the file is
what the search found: no case is constructed by hand."""
import json
import math
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

RR = 0.5
OUT = os.path.join(ROOT, "tests", "golden", "time_column_flips.json")
TRI = np.array([[0.05, 0.0], [-0.025, 0.0433], [-0.025, -0.0433]])     # the obstacle's polygon (bounding circle only)
WANT = 24


def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<q", b))[0]


def _step(x: float, k: int) -> float:
    """the double k places after x in the order of the reals (no zero crossing)"""
    m = _bits(abs(x)) + (k if x >= 0 else -k)
    return math.copysign(_from_bits(m), x)


def edges():
    """long-arc edges near the origin: a pose and the same pose shifted sideways, at three turning radii"""
    for r_min in (2.0, 1.5, 3.0):
        for a in (0.4, 1.3, 2.46, 3.6, 5.1):
            for d in (2.6, 3.0, 3.4):
                for sgn in (-1.0, 1.0):
                    b = a + sgn * 1.71
                    s = np.array([0.3, -0.2, 20.0, a])
                    g = np.array([0.3 + d * r_min * math.cos(b), -0.2 + d * r_min * math.sin(b), 16.0, a + 0.3])
                    yield s, g, r_min


def search():
    cases = []
    cx, cy, rad = O.polygon_ctor(TRI)
    rr = rad + RR
    for s, g, r_min in edges():
        tr_rs = O.dubins_steer_time(s, g, r_min)[4]
        tr_pw = O.dubins_steer_time(s, g, r_min, piecewise=True)[4]
        P = len(tr_rs)
        rows = [i for i in range(20, P - 3) if tr_rs[i, 2] != tr_pw[i, 2] or tr_rs[i + 1, 2] != tr_pw[i + 1, 2]]
        for i in rows[:: max(1, len(rows) // 6)]:
            a, b, c = tr_rs[i - 1, :2], tr_rs[i, :2], tr_rs[i + 1, :2]
            ch = c - b
            L = math.hypot(*ch)
            if not (0.05 * r_min < L < 0.11 * r_min):
                continue                                   # a junction, not a step of an arc
            n = np.array([-ch[1], ch[0]]) / L
            if np.dot(n, (a + c) / 2 - b) < 0:             # towards the inside of the arc
                n = -n
            if abs(n[0]) < 0.3:
                continue
            mid = (b + c) / 2
            t_mid = 0.5 * (tr_rs[i, 2] + tr_rs[i + 1, 2])
            v = 0.02                                       # the obstacle crosses the piece's normal at this speed
            path = np.zeros((2, 3))
            ps = O.PolygonSet([TRI], kinds=[6], paths=[path])
            live = ps.paths[0]

            def put(dx0):
                for k, dt in enumerate((-40.0, 40.0)):
                    live[k] = (dx0 - cx + n[0] * v * dt, mid[1] + n[1] * rr - cy + n[1] * v * dt, t_mid + dt)

            def piece(tr):
                return O.edge_check_polygons(ps, tr[i], tr[i + 1], RR)[0]

            x_in, x_out = mid[0] + n[0] * (rr - 2e-3), mid[0] + n[0] * (rr + 2e-3)
            put(x_in)
            if not piece(tr_rs):
                continue
            put(x_out)
            if piece(tr_rs):
                continue
            lo, hi = x_in, x_out                           # piece(lo) hits, piece(hi) does not
            while abs(_bits(lo) - _bits(hi)) > 1:
                m = _from_bits((_bits(lo) + _bits(hi)) // 2)
                put(m)
                if piece(tr_rs):
                    lo = m
                else:
                    hi = m
            for k in range(-48, 49):
                x = _step(lo, k)
                put(x)
                if piece(tr_rs) == piece(tr_pw):
                    continue
                h_rs = O.dubins_edge_check_polygons_time(ps, s, g, tr_rs, RR, r_min)[0]
                h_pw = O.dubins_edge_check_polygons_time(ps, s, g, tr_pw, RR, r_min)[0]
                if h_rs != h_pw:
                    cases.append(dict(s=s.tolist(), g=g.tolist(), r_min=r_min, polygon=TRI.tolist(), path=live.tolist(),
                                      row=i, rows=P, hit_running_sum=bool(h_rs), hit_piecewise=bool(h_pw)))
                    break
            if len(cases) >= WANT:
                return cases
    return cases


if __name__ == "__main__":
    found = search()
    print(len(found), "cases;", sum(c["hit_running_sum"] for c in found), "of them hit under the running sum")
    with open(OUT, "w") as f:
        json.dump(dict(robot_radius=RR, cases=found), f, indent=0)
