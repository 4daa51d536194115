"""The packed obstacle tables (SphereTableBlock, PolygonTableBlock, PolygonGridBlock of csrc/block_layout.hpp; one
allocation, one upload and one view per list): ONE context per dimension is driven through list after list without being
created again, and after every list its answers are held to the oracle (np.array_equal) and to a context created for
that list alone -- a table, a count or a pointer left over from the list before shows as a difference to either.

The lists sit where the packing can go wrong: sphere counts at the groups of 8 and the pairs of the fp32 reach table
(0, 1, 8, 9, 16, 17), two robot radii over one list, a sphere of infinite reach, spheres switched off and on; polygon
counts at the kernels' groups of 32 and the grid's threshold of 64 (0, 1, 31 .. 33, 63 .. 65; the 512 points are enough
for the grid to be built), a NaN vertex (no y table), no kind-3 polygon in use (an empty y table), every polygon
switched off after a list that had some (the empty list's null view), a list that outgrows the buffer's first block and
a short one after it; in [x y t theta] the moving kinds with a one-row and a five-row path.

Every list is compared with the oracle on a sample of the calls (the polygon point and edge checks, the sphere edge
check), one list per family on all of them: edges_check (hit and first hit, both kinds), points_check flag-only and
with the clearance (both kinds), extend_candidates against the spheres and against the polygons, obstacle_sweep, the
sphere release and the polygon sweep of a burst, dubins_edges_check."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR, DELTA, RMIN, R_EXT = 0.5, 3.0, 2.0, 2.5
N3, NE3, NP3, NQ3 = 2000, 256, 512, 48
N4, NE4 = 500, 128
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")


# ---- the fixed part: nodes, edges, points, samples ------------------------------------------------------------------------
class Fixed3:
    def __init__(self, oracle):
        rng = np.random.default_rng(2024)
        self.pts = np.c_[rng.uniform(-20, 20, (N3, 2)), rng.uniform(-1, 1, N3)]
        self.es = rng.integers(0, N3, NE3).astype(np.int32)
        want = self.pts[self.es] + np.c_[rng.normal(0, 5.0, (NE3, 2)), np.zeros(NE3)]
        self.ee = np.array([int(np.argmin(((self.pts - w) ** 2).sum(1))) for w in want], dtype=np.int32)
        self.ee[0] = self.es[0]                                   # a zero-length edge
        self.p0, self.p1 = self.pts[self.es], self.pts[self.ee]
        self.points = np.c_[rng.uniform(-20, 20, (NP3, 2)), rng.uniform(-1, 1, NP3)]
        self.Q = np.c_[rng.uniform(-18, 18, (NQ3, 2)), rng.uniform(-1, 1, NQ3)]
        self.tree = oracle.KDTree(3)
        self.tree.insert_many(self.pts)
        self.range = oracle.range_batch(self.tree, self.Q, R_EXT)   # the searches do not depend on the lists: once


class Fixed4:
    def __init__(self):
        rng = np.random.default_rng(77)
        self.pts = np.c_[rng.uniform(-20, 20, (N4, 2)), rng.uniform(5, 35, N4), rng.uniform(0, 2 * math.pi, N4)]
        self.S = self.pts[:NE4].copy()
        self.G = self.S.copy()
        self.G[:, :2] += rng.normal(0, 6.0, (NE4, 2))
        self.G[:, 2] -= rng.uniform(0.05, 4.0, NE4)               # planning runs in reverse time
        self.G[:, 3] = rng.uniform(0, 2 * math.pi, NE4)


@pytest.fixture(scope="module")
def fixed3(oracle):
    return Fixed3(oracle)


@pytest.fixture(scope="module")
def fixed4():
    return Fixed4()


def _new3(f):
    ctx = Context(3)
    ctx.nodes_append(f.pts)
    assert ctx.graph_edges_append(f.es, f.ee) == 0
    return ctx


def _new4(f):
    ctx = Context(4)
    ctx.set_wrap(3, 2 * math.pi)
    ctx.set_space_has_time(True)
    ctx.nodes_append(f.pts)
    return ctx


@pytest.fixture(scope="module")
def ctx3(fixed3):
    """THE dim = 3 context: every test of this module leaves its last list in it for the next"""
    with _new3(fixed3) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def ctx4(fixed4):
    with _new4(fixed4) as ctx:
        yield ctx


# ---- the lists a context holds -----------------------------------------------------------------------------------------
class Lists:
    def __init__(self, sph=None, sph_act=None, polys=(), kinds=None, poly_act=None, paths=None, rr=RR):
        self.sph = np.zeros((0, 4)) if sph is None else np.asarray(sph, dtype=np.float64).reshape(-1, 4)
        self.sph_act = np.ones(len(self.sph), dtype=np.uint8) if sph_act is None else np.asarray(sph_act, dtype=np.uint8)
        self.polys = list(polys)
        m = len(self.polys)
        self.kinds = [3] * m if kinds is None else list(kinds)
        self.poly_act = np.ones(m, dtype=np.uint8) if poly_act is None else np.asarray(poly_act, dtype=np.uint8)
        self.paths = [None] * m if paths is None else list(paths)
        self.rr = rr
        # the polygons whose sweep is asked for: those whose centre is a number (a sweep is a range search around it)
        self.swept = np.array([j for j in range(m) if np.isfinite(self.polys[j]).all()], dtype=np.int32)

    def but(self, **kw):
        d = dict(sph=self.sph, sph_act=self.sph_act, polys=self.polys, kinds=self.kinds, poly_act=self.poly_act,
                 paths=self.paths, rr=self.rr)
        d.update(kw)
        return Lists(**d)

    def send_spheres(self, ctx):
        ctx.spheres_set(self.sph, self.sph_act)

    def send_polygons(self, ctx):
        ctx.polygons_set(self.polys, kinds=self.kinds, active=self.poly_act, paths=self.paths)

    def send_sphere_flags(self, ctx):             # rrtx_obstacle_update: the list stays, radius and flag of one entry
        for i in range(len(self.sph)):
            ctx.obstacle_update(i, float(self.sph[i, 3]), bool(self.sph_act[i]))

    def send_polygon_flags(self, ctx):            # rrtx_polygons_set_active: shapes and paths stay
        ctx.polygons_set_active(np.arange(len(self.polys)), self.poly_act)

    def spheres(self, oracle, only=None, without=()):
        """make_spheres of the list; only: that entry alone, in use whatever its flag; without: those switched off"""
        if only is not None:
            return oracle.make_spheres(self.sph[only][None, :])
        act = self.sph_act.copy()
        act[list(without)] = 0
        return oracle.make_spheres(self.sph, act)

    def polygon_set(self, oracle):
        return oracle.PolygonSet(self.polys, kinds=self.kinds, active=self.poly_act, paths=self.paths)


def _spheres(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-18, 18, (n, 2)), rng.uniform(-1, 1, n), rng.uniform(1.0, 3.0, n)]


def _polygons(n, seed=2, verts=None, size=(1.0, 2.5)):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.uniform(-18, 18, 2)
        k = verts or int(rng.integers(3, 7))
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        out.append(c + np.c_[np.cos(ang), np.sin(ang)] * rng.uniform(*size))
    return out


TRIANGLES = _polygons(3, seed=9, verts=3)
NINE = _spheres(9, seed=4)


# ---- what a context answers, and what the oracle does ------------------------------------------------------------------
def _blocked(f):
    return np.arange(0, NE3, 2, dtype=np.int32)          # the edges the release calls find blocked


def _range(L, j):
    """the search range of sphere j's sweep (a caller's number: kept finite for the sphere of infinite radius)"""
    return L.rr + DELTA + min(float(L.sph[j, 3]), 40.0)


def _device3(ctx, f, L):
    """every call of the module against the lists the context holds, as {name: array}"""
    out = {}
    for kind, name in ((0, "sph"), (1, "poly")):
        out[f"edges_{name}_hit"], out[f"edges_{name}_first"] = ctx.edges_check(f.p0, f.p1, L.rr, kind=kind)
        out[f"points_{name}_flag"], none = ctx.points_check(f.points, L.rr, kind=kind, want_clearance=False)
        assert none is None
        out[f"points_{name}_unsafe"], out[f"points_{name}_clr"] = ctx.points_check(f.points, L.rr, kind=kind)
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, kind)
        ext = ctx.extend_candidates(f.Q, R_EXT, L.rr)
        for k in EXTEND_FIELDS:
            out[f"extend_{name}_{k}"] = ext[k]
    ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 0)
    for j in range(len(L.sph)):
        out[f"sweep_sph_{j}"] = ctx.obstacle_sweep(j, _range(L, j), L.rr)
    if len(L.sph):
        burst = np.arange(0, len(L.sph), 3, dtype=np.int32)
        ctx.graph_edges_block(_blocked(f))
        out["release_sph_off"], out["release_sph_ids"] = ctx.obstacle_release_batch(burst, [_range(L, j) for j in burst], L.rr)
        ctx.graph_edges_unblock(_blocked(f))
    if len(L.swept):
        out["sweep_poly_off"], out["sweep_poly_ids"] = ctx.obstacle_sweep_polygon_batch(L.swept, L.rr, DELTA)
    return out


def _oracle3(oracle, f, L, full):
    """the same names from the oracle: all of them (full) or the sample that is compared at every list"""
    out = {}
    ps, sph = L.polygon_set(oracle), L.spheres(oracle)
    out["edges_poly_hit"], out["edges_poly_first"] = oracle.edges_check_batch(ps, f.p0, f.p1, L.rr)
    out["points_poly_unsafe"], out["points_poly_clr"] = oracle.points_check_batch(ps, f.points, L.rr)
    out["points_poly_flag"] = out["points_poly_unsafe"]
    out["edges_sph_hit"], out["edges_sph_first"] = oracle.edges_check_batch(sph, f.p0, f.p1, L.rr)
    if not full:
        return out
    out["points_sph_unsafe"], out["points_sph_clr"] = oracle.points_check_batch(sph, f.points, L.rr)
    out["points_sph_flag"] = out["points_sph_unsafe"]
    for obs, name in ((sph, "sph"), (ps, "poly")):
        ext = oracle.extend_candidates_batch(None, f.Q, R_EXT, f.pts, obs, L.rr, rng=f.range)
        for k in EXTEND_FIELDS:
            out[f"extend_{name}_{k}"] = ext[k]

    def near(j):                                     # edges that start within the sweep's range of sphere j
        idx, _ = f.tree.within_range(_range(L, j), L.sph[j, :3])
        mask = np.zeros(N3, dtype=bool)
        mask[idx] = True
        return mask[f.es]

    for j in range(len(L.sph)):
        hit, _ = oracle.edges_check_batch(L.spheres(oracle, only=j), f.p0, f.p1, L.rr)
        out[f"sweep_sph_{j}"] = np.flatnonzero(near(j) & (hit != 0) & bool(L.sph_act[j])).astype(np.int32)
    if len(L.sph):
        burst = list(range(0, len(L.sph), 3))
        blocked = np.zeros(NE3, dtype=bool)
        blocked[_blocked(f)] = True
        stays, _ = oracle.edges_check_batch(L.spheres(oracle, without=burst), f.p0, f.p1, L.rr)
        rows = []
        for j in burst:
            hit, _ = oracle.edges_check_batch(L.spheres(oracle, only=j), f.p0, f.p1, L.rr)
            rows.append(np.flatnonzero(blocked & near(j) & (hit != 0) & (stays == 0)).astype(np.int32))
        out["release_sph_off"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        out["release_sph_ids"] = np.concatenate(rows).astype(np.int32)
    if len(L.swept):
        rows = [oracle.add_new_obstacle_edges(f.tree, f.pts, f.es, f.ee, ps, j, L.rr, DELTA, dubins=False)
                if L.poly_act[j] else np.zeros(0, dtype=np.int32) for j in L.swept]
        out["sweep_poly_off"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        out["sweep_poly_ids"] = np.concatenate(rows).astype(np.int32)
    return out


def _same(got, want, label):
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (label, k, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (label, k, int((a != b).sum()))


def _hold3(oracle, ctx, f, L, label, full=False):
    """the long-lived context holds L: its answers against the oracle and against a context made for L alone"""
    got = _device3(ctx, f, L)
    _same(got, _oracle3(oracle, f, L, full), label + " against the oracle")
    with _new3(f) as fresh:
        L.send_spheres(fresh)
        L.send_polygons(fresh)
        alone = _device3(fresh, f, L)
    assert sorted(alone) == sorted(got)
    _same(got, alone, label + " against a fresh context")
    return got


# ---- spheres -------------------------------------------------------------------------------------------------------------
def test_sphere_counts_at_the_reach_groups(oracle, ctx3, fixed3):
    base = Lists(polys=TRIANGLES)
    base.send_polygons(ctx3)
    hits = 0
    for n in (17, 0, 1, 8, 9, 16, 17, 0):
        L = base.but(sph=_spheres(17, seed=1)[:n], sph_act=None)
        L.send_spheres(ctx3)
        got = _hold3(oracle, ctx3, fixed3, L, f"{n} spheres", full=(n == 9))
        hits += int(got["edges_sph_hit"].sum())
        if n == 0:
            assert not got["edges_sph_hit"].any() and not got["points_sph_unsafe"].any() and not got["extend_sph_hit_out"].any()
    assert hits > 100


def test_two_robot_radii_over_one_sphere_list(oracle, ctx3, fixed3):
    L = Lists(sph=NINE, polys=TRIANGLES)
    L.send_spheres(ctx3)
    L.send_polygons(ctx3)
    seen = []
    for i, rr in enumerate((0.5, 1.75, 0.5, 1.75)):      # the list is not sent again: the tables follow the radius
        got = _hold3(oracle, ctx3, fixed3, L.but(rr=rr), f"robot radius {rr}", full=(i == 1))
        seen.append(int(got["edges_sph_hit"].sum()))
    assert seen[0] == seen[2] < seen[1] == seen[3]


def test_sphere_of_infinite_reach(oracle, ctx3, fixed3):
    sph = NINE.copy()
    sph[4, 3] = np.inf
    L = Lists(sph=sph, polys=TRIANGLES)
    L.send_spheres(ctx3)
    L.send_polygons(ctx3)
    got = _hold3(oracle, ctx3, fixed3, L, "a sphere of infinite radius", full=True)
    assert got["edges_sph_hit"].all() and (got["edges_sph_first"] <= 4).all()
    L = L.but(sph=NINE)
    L.send_spheres(ctx3)
    assert not _hold3(oracle, ctx3, fixed3, L, "the finite list after it")["edges_sph_hit"].all()


def test_sphere_flags_off_and_on(oracle, ctx3, fixed3):
    L = Lists(sph=_spheres(17, seed=1), polys=TRIANGLES)
    L.send_spheres(ctx3)
    L.send_polygons(ctx3)
    _hold3(oracle, ctx3, fixed3, L, "17 spheres in use")
    for label, act, full in (("every second sphere off", np.arange(17) % 2, True), ("all spheres off", np.zeros(17), False),
                             ("all spheres on again", np.ones(17), False)):
        L = L.but(sph_act=act.astype(np.uint8))
        L.send_sphere_flags(ctx3)
        got = _hold3(oracle, ctx3, fixed3, L, label, full=full)
        assert got["edges_sph_hit"].any() == bool(act.any())


# ---- polygons ------------------------------------------------------------------------------------------------------------
def test_polygon_counts_at_the_groups_and_the_grid(oracle, ctx3, fixed3):
    base = Lists(sph=NINE)
    base.send_spheres(ctx3)
    every = _polygons(65, seed=2)
    hits = 0
    for n in (65, 0, 1, 31, 32, 33, 63, 64, 65, 1):
        L = base.but(polys=every[:n], kinds=None, poly_act=None, paths=None)
        L.send_polygons(ctx3)
        got = _hold3(oracle, ctx3, fixed3, L, f"{n} polygons", full=(n == 33))
        hits += int(got["edges_poly_hit"].sum())
        if n == 0:
            assert not got["edges_poly_hit"].any() and not got["points_poly_flag"].any() and not got["extend_poly_hit_in"].any()
    assert hits > 200


def test_polygon_list_without_a_y_table(oracle, ctx3, fixed3):
    """a NaN vertex: no table (n_ytab = -1); then no kind-3 polygon in use: an empty table (n_ytab = 0)"""
    base = Lists(sph=NINE)
    base.send_spheres(ctx3)
    polys = _polygons(12, seed=6)
    nan = [p.copy() for p in polys]
    nan[5][1, 1] = np.nan
    L = base.but(polys=nan, kinds=None, poly_act=None, paths=None)
    L.send_polygons(ctx3)
    _hold3(oracle, ctx3, fixed3, L, "a NaN vertex", full=True)
    kinds = [1] * 12
    kinds[7] = 3
    act = np.ones(12, dtype=np.uint8)
    act[7] = 0
    L = base.but(polys=polys, kinds=kinds, poly_act=act, paths=None)
    L.send_polygons(ctx3)
    got = _hold3(oracle, ctx3, fixed3, L, "the only kind-3 polygon not in use")
    assert got["points_poly_flag"].any()
    L = base.but(polys=polys, kinds=None, poly_act=None, paths=None)
    L.send_polygons(ctx3)
    _hold3(oracle, ctx3, fixed3, L, "twelve kind-3 polygons after it")


def test_polygon_flags_all_off_then_three_on(oracle, ctx3, fixed3):
    """the empty list after a list that had tables: m = 0 and a null view, the same kernel as a list never filled"""
    base = Lists(sph=NINE, polys=_polygons(40, seed=8))
    base.send_spheres(ctx3)
    base.send_polygons(ctx3)
    _hold3(oracle, ctx3, fixed3, base, "40 polygons in use")
    off = base.but(poly_act=np.zeros(40, dtype=np.uint8))
    off.send_polygon_flags(ctx3)
    got = _hold3(oracle, ctx3, fixed3, off, "all polygons off", full=True)
    for k in ("edges_poly_hit", "points_poly_flag", "points_poly_unsafe", "extend_poly_hit_out", "extend_poly_hit_in",
              "extend_poly_sample_unsafe", "sweep_poly_ids"):
        assert not got[k].any(), k
    act = np.zeros(40, dtype=np.uint8)
    act[[3, 20, 39]] = 1
    on = base.but(poly_act=act)
    on.send_polygon_flags(ctx3)
    got = _hold3(oracle, ctx3, fixed3, on, "three polygons on")
    assert set(got["edges_poly_first"][got["edges_poly_hit"] != 0].tolist()) <= {3, 20, 39} and got["edges_poly_hit"].any()


def test_polygon_buffer_moves_and_shrinks(oracle, ctx3, fixed3):
    """3 triangles fit the buffer's first 4 096 bytes; 300 polygons of 12 vertices do not, so it is allocated again"""
    base = Lists(sph=NINE)
    base.send_spheres(ctx3)
    many = _polygons(300, seed=12, verts=12, size=(0.4, 0.9))
    for label, polys, full in (("3 triangles", TRIANGLES, False), ("300 polygons of 12", many, True),
                               ("3 triangles again", TRIANGLES, False)):
        L = base.but(polys=polys, kinds=None, poly_act=None, paths=None)
        L.send_polygons(ctx3)
        got = _hold3(oracle, ctx3, fixed3, L, label, full=full)
        assert got["edges_poly_hit"].any()


# ---- [x y t theta]: the moving kinds ------------------------------------------------------------------------------------------
def _device4(ctx, f):
    cost, word, hit, tl = ctx.dubins_edges_check(f.S, f.G, RMIN, RR)
    return dict(cost=cost, word=word, hit=hit, traj_len=tl)


def test_moving_polygons_in_space_with_time(oracle, ctx4, fixed4):
    polys = _polygons(9, seed=21, size=(2.0, 4.0))
    rng = np.random.default_rng(3)
    one_row = np.array([[4.0, -3.0, 20.0]])
    five_rows = np.c_[rng.uniform(-12, 12, (5, 2)), np.sort(rng.uniform(0, 36, 5))]
    kinds = [3, 6, 3, 7, 3, 3, 6, 3, 3]
    paths = [None, one_row, None, five_rows, None, None, five_rows[::1] * [1.0, -1.0, 1.0], None, None]
    lists = [("static polygons", Lists(polys=polys[:3])),
             ("kinds 6 and 7", Lists(polys=polys, kinds=kinds, paths=paths)),
             ("all off", Lists(polys=polys, kinds=kinds, paths=paths, poly_act=np.zeros(9, dtype=np.uint8))),
             ("kinds 6 and 7 again", Lists(polys=polys, kinds=kinds, paths=paths)),
             ("one moving polygon", Lists(polys=polys[1:2], kinds=[6], paths=[one_row]))]
    hits = []
    for label, L in lists:
        if label == "all off":
            L.send_polygon_flags(ctx4)
        else:
            L.send_polygons(ctx4)
        got = _device4(ctx4, fixed4)
        ref = oracle.dubins_edges_batch(fixed4.S, fixed4.G, RMIN, L.polygon_set(oracle), RR, has_time=True, piecewise=True)
        _same(got, {k: ref[k] for k in got}, label + " against the oracle")
        with _new4(fixed4) as fresh:
            L.send_polygons(fresh)
            _same(got, _device4(fresh, fixed4), label + " against a fresh context")
        hits.append(int(got["hit"].sum()))
    assert hits[0] > 0 and hits[1] > 0 and hits[2] == 0 and hits[3] == hits[1]
