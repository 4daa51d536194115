"""include/rrtx.h promises of the tuning switches of rrtx_set_option that "none of them changes a result".  They fix the
shape of every launch of the range search: copies per tile, node segments and the persistent grid of the brute-force
scans (RRTX_OPT_SCAN_TILE_Q / _ITEMS / _BLOCKS), the bucket grid and the slab index of the culled search
(RRTX_OPT_TUNE), the width of the per-query hit buckets (RRTX_OPT_BUCKET_MULT), and which launches carry events
(rrtx_profile, RRTX_OPT_PROFILE_EVERY).  This file walks those shapes on trees of 9 001 and 20 011 nodes -- no multiple
of 512, 1024 or 2048, so last tiles and last segments are partial -- and holds every configuration, the default one
included, to the CPU oracle with np.array_equal on offsets, indices, stored distances and flags.  No device run is
compared with another device run.

Every configuration must also show that its switch reached the launch: a restatement of plan_radius (kernels_nn.hip)
says which corner a configuration is (asserted here, on the restatement), and stats().last_tile_q,
stats().last_scan_units and RRTX_OPT_LAST_PLACEMENT say what the library did.

Scenes
  A  dim 3, no wraps: 18 800 nodes uniform in the world box and 1 211 in a cluster of sigma 0.8 (20 011 in all), radius
     synth.ball_radius; 70 uniform queries, one on a node, one far outside the cloud (empty list), one with a NaN
     coordinate and six in the cluster (lists of more than 1 000 nodes at the scene's one radius, which the fused
     extend() call needs); 24 spheres, one of them inside the cluster; 700 more nodes to append (a tail of the slab index).
  B  dim 4, theta wrapped with period 2 pi: 9 001 nodes, 60 queries, six of them with theta next to 0 and 2 pi; two
     copies per query, so the culled search takes the place route.  16 polygons for the Dubins preamble.
  C  scene A's nodes, 2 500 queries: the bucket grid, the slots per bucket and the spill list of the slot route move.
"""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

from test_find_target_reference import KEYS, Scene, find_target_batch

pytestmark = pytest.mark.gpu

RR = 0.5
TWO_PI = 2.0 * math.pi
OPT = _capi
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- scenes and their oracle results (computed once per module, never modified) -------------------------------------
CLUSTER = np.array([12.0, -7.0, 20.0])


def scene_a():
    def make():
        rng = np.random.default_rng(77)
        pts = np.concatenate([synth.nodes(18_800, 3), CLUSTER + rng.normal(0.0, 0.8, (1_211, 3))])
        pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
        Q = np.concatenate([synth.queries(70, 3), pts[137:138], [[400.0, 400.0, 400.0]], [[3.0, np.nan, -4.0]],
                            CLUSTER + rng.normal(0.0, 0.5, (6, 3))])
        extra = synth.nodes(700, 3, seed=5)
        sph = synth.spheres(24)
        sph[0] = [CLUSTER[0] + 1.2, CLUSTER[1] + 0.5, CLUSTER[2] - 0.3, 1.0]       # one obstacle inside the cluster
        assert len(pts) == 20_011 and len(pts) % 512 and len(pts) % 2048
        return dict(dim=3, pts=pts, Q=np.ascontiguousarray(Q), r=synth.ball_radius(len(pts), 3), sph=sph,
                    extra=extra, on_node=70, outside=71, nan=72, dense=np.arange(73, 79))
    return _once("A", make)


def scene_b():
    def make():
        pts = synth.nodes(9_001, 4)
        Q = synth.queries(60, 4).copy()
        Q[:6, 3] = [0.0, 0.01, 1.0, TWO_PI - 0.01, TWO_PI - 1.0, 6.2]
        return dict(dim=4, pts=pts, Q=np.ascontiguousarray(Q), r=2.5, polys=synth.polygons(16), r_min=1.0)
    return _once("B", make)


def scene_c():
    a = scene_a()
    return _once("C", lambda: dict(dim=3, pts=a["pts"], Q=synth.queries(2_500, 3, seed=31), r=a["r"]))


def trees_of(oracle, name, appended=False):
    def make():
        if name == "B":
            return oracle.TreeSet(4, scene_b()["pts"], wraps=[3], wrap_points=[TWO_PI])
        a = scene_a()
        return oracle.TreeSet(3, np.concatenate([a["pts"], a["extra"]]) if appended else a["pts"])
    return _once(("trees", "A" if name == "C" else name, appended), make)


def scene(name):
    return {"A": scene_a, "B": scene_b, "C": scene_c}[name]()


def ref_lists(oracle, name, appended=False):
    """the oracle's range lists (ascending node index) and kdFindNearest of the scene's queries"""
    s = scene(name)
    return _once(("lists", name, appended), lambda: oracle.range_batch(trees_of(oracle, name, appended), s["Q"], s["r"]))


def ref_extend(oracle, appended=False):
    """what rrtx_extend_candidates returns on scene A, from the oracle: the lists, explicitEdgeCheck of both directed
    edges of every entry (edges_check_spheres over synth.candidate_edges) and explicitPointCheck of every sample"""
    def make():
        a = scene_a()
        pts = np.concatenate([a["pts"], a["extra"]]) if appended else a["pts"]
        rng = ref_lists(oracle, "A", appended)
        p0, p1 = synth.candidate_edges(a["Q"], pts, rng["offsets"], rng["idx"])
        arr, m = oracle.make_spheres(a["sph"])
        hit, _ = oracle.edges_check_spheres(arr, m, p0, p1, RR)
        unsafe, _ = oracle.points_check_spheres(arr, m, a["Q"], RR)
        n = len(rng["idx"])
        return dict(offsets=rng["offsets"], idx=rng["idx"], cost=rng["key"], hit_out=hit[:n], hit_in=hit[n:],
                    nearest_idx=rng["nearest_idx"], nearest_dist=rng["nearest_dist"], sample_unsafe=unsafe)
    return _once(("extend", appended), make)


def test_scenes_reach_the_edges(oracle):
    """the properties of the scenes the other tests rely on, judged on the oracle alone"""
    a, ref = scene_a(), ref_lists(oracle, "A")
    n = np.diff(ref["offsets"])
    assert n[a["on_node"]] > 0 and ref["key"][ref["offsets"][a["on_node"]]:ref["offsets"][a["on_node"] + 1]].min() == 0.0
    assert n[a["outside"]] == 0 and n[a["nan"]] == 0
    assert (n[a["dense"]] > 1000).all() and np.median(n) < 64
    ext = ref_extend(oracle)
    assert 0 < ext["hit_out"].sum() < len(ext["hit_out"]) and 0 < ext["sample_unsafe"].sum() < len(a["Q"])
    assert (np.diff(ref_lists(oracle, "A", True)["offsets"]) >= n).all()
    assert ref_lists(oracle, "A", True)["offsets"][-1] > ref["offsets"][-1]          # the appended tail holds neighbours
    b, refb = scene_b(), ref_lists(oracle, "B")
    plain = oracle.range_batch(oracle.TreeSet(4, b["pts"]), b["Q"], b["r"], nearest=False)
    gained = np.diff(refb["offsets"]) - np.diff(plain["offsets"])
    assert (gained >= 0).all() and (gained[:6] > 0).sum() >= 4 and (gained > 0).sum() >= 12     # ghosts find neighbours
    c = ref_lists(oracle, "C")
    assert c["offsets"][-1] > 10 * 2_500


# ---- the device side --------------------------------------------------------------------------------------------------
def make_ctx(name, options=(), appended=False):
    """a fresh context holding the scene, the options set before the first search (and before the index is built)"""
    s = scene(name)
    ctx = Context(s["dim"])
    try:
        for opt, val in options:
            ctx.set_option(opt, val)
        if s["dim"] == 4:
            ctx.set_wrap(3, TWO_PI)
            ctx.polygons_set(s["polys"])
        ctx.nodes_append(s["pts"])
        if name == "A":
            ctx.spheres_set(s["sph"])
        if appended:
            ctx.nodes_append(s["extra"])
    except Exception:
        ctx.close()
        raise
    return ctx


def assert_lists(got, ref, label):
    off, idx, dist = got
    assert np.array_equal(off, ref["offsets"]), f"{label}: offsets"
    assert np.array_equal(idx, ref["idx"]), f"{label}: idx"
    assert np.array_equal(dist, ref["key"]), f"{label}: dist"


def radius_vs_oracle(oracle, ctx, name, label, appended=False):
    s, ref = scene(name), ref_lists(oracle, name, appended)
    assert_lists(ctx.nn_radius(s["Q"], s["r"], cap=len(ref["idx"]) + 64), ref, f"{label} nn_radius scene {name}")


def extend_vs_oracle(oracle, ctx, label, appended=False):
    a, ref = scene_a(), ref_extend(oracle, appended)
    out = ctx.extend_candidates(a["Q"], a["r"], RR, cap=len(ref["idx"]) + 64)
    for k in ("offsets", "idx", "cost", "hit_out", "hit_in", "sample_unsafe"):
        assert np.array_equal(out[k], ref[k]), f"{label} extend_candidates: {k}"
    # a sample with a NaN coordinate orders against no node: the device answers (INT_MAX, inf) where kdFindNearest
    # keeps its seed (root, NaN); every other sample has the oracle's nearest node
    keep = np.arange(len(a["Q"])) != a["nan"]
    assert np.array_equal(out["nearest_idx"][keep], ref["nearest_idx"][keep]), f"{label} extend_candidates: nearest_idx"
    assert np.array_equal(out["nearest_dist"][keep], ref["nearest_dist"][keep]), f"{label} extend_candidates: nearest_dist"
    assert out["nearest_idx"][a["nan"]] == 0x7fffffff and np.isinf(out["nearest_dist"][a["nan"]])


# ---- plan_radius restated (kernels_nn.hip): the sizes of the brute-force scans -------------------------------------
def _ceil(a, b):
    return (a + b - 1) // b


def scan_plan(n_nodes, n_copies_max, screened, tile_q_opt=0, items_opt=2048, blocks_opt=1280):
    tile_q = 64 if screened else 32
    if tile_q_opt > 0:
        tile_q = _ceil(tile_q_opt, 4) * 4
    if screened and tile_q > 128:
        tile_q = 128
    n_tiles = _ceil(n_copies_max, tile_q)
    chunk = 512 if screened else 256            # nodes per wave per pass; a workgroup of four waves covers 4 chunks
    max_seg = _ceil(n_nodes, 4 * chunk)
    want_seg = _ceil(items_opt if screened else 4096, n_tiles)
    n_seg = max(1, min(want_seg, max_seg))
    if n_seg >= 8:
        n_seg = n_seg // 8 * 8
    seg_len = _ceil(_ceil(n_nodes, n_seg), chunk) * chunk
    n_seg = _ceil(n_nodes, seg_len)
    n_items = n_tiles * n_seg
    grid = min(n_items, max(8, blocks_opt // 8 * 8)) if screened else n_items
    return dict(tile_q=tile_q, n_tiles=n_tiles, n_seg=n_seg, seg_len=seg_len, n_items=n_items, grid=grid,
                partial_tile=n_copies_max % tile_q != 0, partial_seg=n_nodes % seg_len != 0)


def _sizes(name):
    s = scene(name)
    return len(s["pts"]), len(s["Q"]) * (2 if s["dim"] == 4 else 1)


# (SCAN_TILE_Q, SCAN_ITEMS, SCAN_BLOCKS), None = left at its default
SCREENED = [(None, None, None), (4, 100_000, 1), (1, 1, 8), (6, 2048, 20), (20, 2048, 1280), (64, 1, 1),
            (128, 100_000, 1280), (1000, 2048, 8)]


def _screened_plan(name, cfg):
    tq, items, blocks = cfg
    return scan_plan(*_sizes(name), True, tq or 0, items or 2048, blocks or 1280)


def test_screened_configurations_cover_the_corners():
    """the corners the list above must contain, decided on the restated plan (scene A has one copy per query, so its
    copy count is known; scene B's depends on which ghosts are in range, so only its node side is judged)"""
    pa = {c: _screened_plan("A", c) for c in SCREENED}
    pb = {c: _screened_plan("B", c) for c in SCREENED}
    assert pa[(None, None, None)]["tile_q"] == 64
    assert any(p["partial_tile"] and p["n_tiles"] > 1 for p in pa.values())
    assert any(p["partial_tile"] and p["n_tiles"] == 1 for p in pa.values())
    assert any(p["n_seg"] == 1 for p in pa.values()) and any(p["n_seg"] == 1 for p in pb.values())
    assert any(1 < p["n_seg"] < 8 and p["partial_seg"] for p in pb.values())
    assert any(p["n_seg"] == 8 and p["partial_seg"] for p in pa.values())
    assert any(p["n_items"] >= 4 * p["grid"] for p in pa.values()) and any(p["n_items"] >= 4 * p["grid"] for p in pb.values())
    assert pa[(1000, 2048, 8)]["tile_q"] == 128 and pa[(1, 1, 8)]["tile_q"] == 4 and pa[(6, 2048, 20)]["tile_q"] == 8
    assert {p["grid"] for p in pa.values()} >= {2, 8, 16}


@pytest.mark.parametrize("cfg", SCREENED, ids=lambda c: "tq{}-items{}-blocks{}".format(*c))
@pytest.mark.parametrize("name", ["A", "B"])
def test_screened_scan_geometry(oracle, name, cfg):
    tq, items, blocks = cfg
    options = [(OPT.RRTX_OPT_NN_CULL, 0), (OPT.RRTX_OPT_NN_FILTER, 1)]
    options += [(o, v) for o, v in ((OPT.RRTX_OPT_SCAN_TILE_Q, tq), (OPT.RRTX_OPT_SCAN_ITEMS, items),
                                    (OPT.RRTX_OPT_SCAN_BLOCKS, blocks)) if v is not None]
    plan = _screened_plan(name, cfg)
    with make_ctx(name, options) as ctx:
        radius_vs_oracle(oracle, ctx, name, f"screened {cfg}")
        st = ctx.stats()
        assert st.last_tile_q == plan["tile_q"]
        assert st.last_scan_units == 0 and ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == 0
        assert st.last_pairs == _sizes(name)[0] * _sizes(name)[1]
        radius_vs_oracle(oracle, ctx, name, f"screened {cfg}, second call")


def test_scan_options_are_normalised():
    with Context(3) as ctx:
        for opt, given, kept in [(OPT.RRTX_OPT_SCAN_BLOCKS, 0, 1280), (OPT.RRTX_OPT_SCAN_BLOCKS, 20, 20),
                                 (OPT.RRTX_OPT_SCAN_ITEMS, 0, 2048), (OPT.RRTX_OPT_SCAN_ITEMS, 100_000, 100_000),
                                 (OPT.RRTX_OPT_SCAN_TILE_Q, -3, 0), (OPT.RRTX_OPT_SCAN_TILE_Q, 6, 6),
                                 (OPT.RRTX_OPT_PROFILE_EVERY, 0, 1), (OPT.RRTX_OPT_PROFILE_EVERY, 3, 3)]:
            ctx.set_option(opt, given)
            assert ctx.get_option(opt) == kept, (opt, given)
        for given, kept in [(2, 2), (4, 4), (8, 8), (16, 16), (0, 2), (5, 8), (99, 16)]:
            ctx.set_option(OPT.RRTX_OPT_BUCKET_MULT, given)
            assert ctx.get_option(OPT.RRTX_OPT_BUCKET_MULT) == kept, given


@pytest.mark.parametrize("tq", [4, 32, 200])
@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_scan_geometry(oracle, name, tq):
    """RRTX_OPT_NN_FILTER = 0: tile_q is not clamped to 128 and RRTX_OPT_SCAN_ITEMS is not read (4096 items)"""
    plan = scan_plan(*_sizes(name), False, tq)
    assert plan["tile_q"] == tq and plan["partial_seg"] and plan["n_seg"] >= 8
    for items in (None, 1, 100_000):
        options = [(OPT.RRTX_OPT_NN_FILTER, 0), (OPT.RRTX_OPT_SCAN_TILE_Q, tq)]
        if items is not None:
            options.append((OPT.RRTX_OPT_SCAN_ITEMS, items))
        with make_ctx(name, options) as ctx:
            radius_vs_oracle(oracle, ctx, name, f"exact tile_q {tq} items {items}")
            st = ctx.stats()
            assert st.last_tile_q == tq and st.last_scan_units == 0
            assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == 0


# ---- the culled search: RRTX_OPT_TUNE --------------------------------------------------------------------------------
XY_ORDER, WHOLE_CHUNKS, PLACE_PASS = 1, 2, 4


def kz(v):
    return v << 8


def g3(v):
    return v << 16


def cs(v):
    return v << 24


TUNES = [0, XY_ORDER, WHOLE_CHUNKS, kz(1), kz(2), kz(7), kz(255), g3(1), g3(2), g3(16), g3(31), cs(1), cs(2), cs(3),
         XY_ORDER | WHOLE_CHUNKS | PLACE_PASS, kz(1) | cs(3)]
COARSER = (WHOLE_CHUNKS, kz(1))       # these list whole chunks where the default lists groups of eight positions


def culled_ctx(name, tune, appended=False):
    return make_ctx(name, [(OPT.RRTX_OPT_NN_CULL, 2), (OPT.RRTX_OPT_TUNE, tune)], appended)


def default_units(oracle, name):
    def make():
        with culled_ctx(name, 0) as ctx:
            radius_vs_oracle(oracle, ctx, name, "default")
            return ctx.stats().last_scan_units
    return _once(("units", name), make)


@pytest.mark.parametrize("tune", TUNES, ids=lambda t: f"tune{t:#x}")
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_culled_search_geometry(oracle, name, tune):
    """Every field of RRTX_OPT_TUNE must also reach the launch.  last_scan_units is the only counter they move, and
    only scene C has enough copies for every field to move it: there each non-default value streams a count of node
    chunks at least 10 % away from the default's (the slots of a bucket are handed out by atomics, so a count can
    differ by a unit or so from run to run, which is why nothing finer, and no equality of bits 16-20 = 16 and 31, is
    asserted).  On scenes A and B some fields leave the count where it was (the bucket grid and the bins of the
    third coordinate do not move the 120 copies of scene B), so there only the coarser listings are compared."""
    route = 1 if (name == "B" or tune & PLACE_PASS) else 2
    with culled_ctx(name, tune) as ctx:
        assert ctx.get_option(OPT.RRTX_OPT_TUNE) == tune
        radius_vs_oracle(oracle, ctx, name, f"tune {tune:#x}")
        st = ctx.stats()
        assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == route
        assert st.last_tile_q == 16 and st.last_scan_units > 0
        base = default_units(oracle, name)
        if tune in COARSER:
            assert st.last_scan_units >= base
        if name == "C" and tune != 0:
            assert st.last_scan_units != base
        radius_vs_oracle(oracle, ctx, name, f"tune {tune:#x}, second call")


@pytest.mark.parametrize("tune", TUNES, ids=lambda t: f"tune{t:#x}")
def test_culled_extend_geometry(oracle, tune):
    """the fused extend() call on scene A (lists, both edge flags of every entry, the sample flags, the nearest node),
    then again with 700 nodes appended behind the sorted part of the slab index"""
    route = 1 if tune & PLACE_PASS else 2
    with culled_ctx("A", tune) as ctx:
        extend_vs_oracle(oracle, ctx, f"tune {tune:#x}")
        assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == route and ctx.stats().last_scan_units > 0
        ctx.nodes_append(scene_a()["extra"])
        assert ctx.n_nodes == 20_711
        extend_vs_oracle(oracle, ctx, f"tune {tune:#x}, appended", appended=True)
        radius_vs_oracle(oracle, ctx, "A", f"tune {tune:#x}, appended", appended=True)
        assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == route and ctx.stats().last_scan_units > 0


# ---- the per-query hit buckets: RRTX_OPT_BUCKET_MULT -------------------------------------------------------------------
def bucket_cap(total, nq, mult):
    """plan_radius: records per query bucket for a caller that made room for `total` entries"""
    return max(8, _ceil(_ceil(total, nq) * mult, 8) * 8)


@pytest.mark.parametrize("cull", [2, 0])
@pytest.mark.parametrize("mult", [2, 4, 8, 16, 0, 5, 99])
def test_bucket_multiplier(oracle, mult, cull):
    """cap = the exact total: buckets of mult x the average list.  The lists of the six dense queries outgrow them at 2
    (their records take the shared overflow list) and fit at 16.  The library learns of an overflow from the finish
    kernel and widens the buckets when the NEXT search is planned, so the growth shows after a second call."""
    a, ref = scene_a(), ref_lists(oracle, "A")
    total, nq, longest = len(ref["idx"]), len(a["Q"]), int(np.diff(ref["offsets"]).max())
    assert longest > bucket_cap(total, nq, 2) and longest <= bucket_cap(total, nq, 16)
    kept = {2: 2, 4: 4, 8: 8, 16: 16, 0: 2, 5: 8, 99: 16}[mult]
    with make_ctx("A", [(OPT.RRTX_OPT_NN_CULL, cull), (OPT.RRTX_OPT_BUCKET_MULT, mult)]) as ctx:
        assert ctx.get_option(OPT.RRTX_OPT_BUCKET_MULT) == kept
        for call in range(2):
            assert_lists(ctx.nn_radius(a["Q"], a["r"], cap=total), ref, f"bucket multiplier {mult}, call {call}")
        now = ctx.get_option(OPT.RRTX_OPT_BUCKET_MULT)
        if kept == 2:
            assert now > 2
        if kept == 16:
            assert now == 16
        assert now >= kept


# ---- profiling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [2, 0])
@pytest.mark.parametrize("level,every", [(0, 1), (1, 1), (1, 3), (2, 1)])
def test_profiling_changes_no_result(oracle, level, every, cull):
    """Six nn_radius calls under every profiling level.  launch_nn_radius opens ONE span of the scan family per call
    (around the tile kernel, or around scan + confirm), so six calls are six scan-family launches.  span_begin counts
    them from the rrtx_profile call on a fresh context (tick 1, 2, ...) and at level 1 times launch t only when
    t % PROFILE_EVERY == 0: with PROFILE_EVERY = 3 launches 3 and 6 of the six, hence launches_nn_scan = 6 // 3 = 2;
    with PROFILE_EVERY = 1 all six.  Level 1 times no other family; level 2 times every span of every family; level 0
    none.  rrtx_stats reports timed launches only."""
    with make_ctx("A", [(OPT.RRTX_OPT_NN_CULL, cull), (OPT.RRTX_OPT_PROFILE_EVERY, every)]) as ctx:
        ctx.profile(level)
        for call in range(6):
            radius_vs_oracle(oracle, ctx, "A", f"profile level {level} every {every}, call {call}")
        st = ctx.stats()
        launches = {k: getattr(st, "launches_" + k) for k in ("nn_scan", "nn_finish", "nn_nearest", "edges", "points",
                                                             "dubins", "dubins_steer")}
        times = {k: getattr(st, "ms_" + k) for k in launches}
        assert all(t >= 0.0 for t in times.values()), times
        if level == 0:
            assert not any(launches.values()), launches
        elif level == 1:
            assert launches["nn_scan"] == 6 // every
            assert not any(v for k, v in launches.items() if k != "nn_scan"), launches
        else:
            assert launches["nn_scan"] == 6 and launches["nn_finish"] > 0


# ---- the other consumers of the range search under two non-default geometries ------------------------------------------
GEOMETRIES = {
    "unculled": [(OPT.RRTX_OPT_NN_CULL, 0), (OPT.RRTX_OPT_SCAN_TILE_Q, 4), (OPT.RRTX_OPT_SCAN_BLOCKS, 8),
                 (OPT.RRTX_OPT_SCAN_ITEMS, 100_000)],
    "culled": [(OPT.RRTX_OPT_NN_CULL, 2), (OPT.RRTX_OPT_TUNE, WHOLE_CHUNKS | kz(2) | cs(2))],
}


def assert_geometry_reached(ctx, geometry, culled_route, streams=True):
    """the context's last range search ran, and under the geometry asked for: a context that never searched reports
    last_pairs 0 and last_tile_q 0, one that ignored RRTX_OPT_SCAN_TILE_Q reports 64.  streams: that last search
    had nodes within reach of its queries (the culled search then counts scan units)"""
    st = ctx.stats()
    assert st.last_pairs > 0
    if geometry == "culled":
        assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == culled_route
        assert st.last_tile_q == 16 and (st.last_scan_units > 0 or not streams)
    else:
        assert ctx.get_option(OPT.RRTX_OPT_LAST_PLACEMENT) == 0
        assert st.last_tile_q == 4 and st.last_scan_units == 0


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_knearest_under_geometry(oracle, geometry):
    """k = 5.  rrtx_nn_knearest takes its answers from range-search lists only for batches of at least 256 queries on a
    culled tree, so the batch is scene A's queries behind 300 of scene C's (same nodes); without culling every query
    runs the exhaustive kernel and the range search is not launched at all (last_pairs stays 0)."""
    a = scene_a()
    Q = np.ascontiguousarray(np.concatenate([scene_c()["Q"][:300], a["Q"]]))
    nan = 300 + a["nan"]
    k = 5
    oi, ok, oc = oracle.knearest_batch(trees_of(oracle, "A"), k, Q)
    order = np.lexsort((oi, ok), axis=1)                               # the device's order: (distance, index)
    oi, ok = np.take_along_axis(oi, order, axis=1), np.take_along_axis(ok, order, axis=1)
    with make_ctx("A", GEOMETRIES[geometry]) as ctx:
        idx, dist, count = ctx.nn_knearest(Q, k)
        assert ctx.stats().last_pairs == (len(Q) * len(a["pts"]) if geometry == "culled" else 0)
    keep = np.arange(len(Q)) != nan
    assert (oc[keep] == k).all() and np.array_equal(count[keep], oc[keep])
    assert np.array_equal(idx[keep], oi[keep]) and np.array_equal(dist[keep], ok[keep])
    assert count[nan] == 0                                             # no node is at a finite distance from it


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_dubins_preamble_under_geometry(oracle, geometry):
    b, rng = scene_b(), ref_lists(oracle, "B")
    ref = oracle.dubins_candidates_batch(b["Q"], rng["offsets"], rng["idx"], b["pts"], b["r_min"],
                                         oracle.PolygonSet(b["polys"]), RR)
    assert 0 < ref["hit_out"].sum() < len(ref["hit_out"])
    with make_ctx("B", GEOMETRIES[geometry]) as ctx:
        out = ctx.extend_candidates_dubins(b["Q"], b["r"], RR, b["r_min"])
        assert_geometry_reached(ctx, geometry, 1)
    assert_lists((out["offsets"], out["idx"], out["key"]), rng, f"Dubins preamble, {geometry}")
    for k in ("cost_out", "cost_in", "hit_out", "hit_in"):
        assert np.array_equal(out[k], ref[k]), (geometry, k)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_find_new_target_under_geometry(oracle, geometry):
    a = scene_a()
    poses = np.ascontiguousarray(np.delete(a["Q"], a["nan"], axis=0))
    sc = Scene("spheres", a["pts"], oracle.make_spheres(a["sph"]), RR)
    lmc = np.random.default_rng(12).uniform(0.0, 60.0, len(a["pts"]))
    lmc[np.random.default_rng(13).random(len(lmc)) < 0.3] = math.inf
    lmc[0] = 0.0
    r0, r_max = 1.5, 30.0
    ref = find_target_batch(oracle, sc, trees_of(oracle, "A"), poses, r0, r_max, lmc)
    assert (ref["rounds"] >= 2).sum() >= 8 and len(set(ref["status"].tolist())) == 2 and (ref["rounds"] == 1).any()
    with make_ctx("A", GEOMETRIES[geometry]) as ctx:
        got = ctx.find_new_target(poses, r0, r_max, RR, lmc=lmc)
        # (the last round is the pose far outside the cloud alone, at r_max: no node cell is within its reach)
        assert ref["rounds"].argmax() == a["outside"] and (ref["rounds"] == ref["rounds"].max()).sum() == 1
        assert_geometry_reached(ctx, geometry, 2, streams=False)
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (geometry, k)
