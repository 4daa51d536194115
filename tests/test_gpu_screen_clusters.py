"""The screened searches on the scenes of tests/screen_model.py: dense clusters far from the context origin, where the
fp32 screen value cannot rank the nodes and the margins of the screens (M of nn_nearest_f32_kernel, thr' of make_qrecf)
decide which nodes reach the exact test.  tests/test_screen_scenes.py shows on a numpy model that the regime is real.

Every comparison is == on indices and on the bit patterns of distances, against the exact fp64 references of
screen_model (unfused sums in the project's order, lowest index on ties, ghosts by torus_model's rule), and where the
oracle has the operation against the oracle as well: KDTree.nearest(naive=True) at every 16th query, range_batch (the
batched kdFindWithinRange) for the range lists, extend_closest_model.closest_reference for the closest-self rows."""
import functools

import numpy as np
import pytest

import extend_closest_model as E
import screen_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
SCENES = M.scenes()
MODES = ("a record for every pair", "default capacity", "capacity 32", "exact scan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _context(pts, meta):
    ctx = Context(meta["dim"])
    for d, per in zip(meta["wraps"], meta["periods"]):
        ctx.set_wrap(d, per)
    ctx.nodes_append(pts)
    return ctx


def _set_mode(ctx, mode, nq, n, n_wraps):
    """the four ways through rrtx_nn_nearest: no record can be lost (the pure screened-confirm path through
    drain_nearest and the tie kernel), the default capacity, 32 records (every query goes to the fix-up kernel), and
    the exact scan"""
    ctx.set_option(_capi.RRTX_OPT_NN_FILTER, 0 if mode == "exact scan" else 1)
    cap = {"a record for every pair": (nq << n_wraps) * n + 4096, "capacity 32": 32}.get(mode, 0)
    ctx.set_option(_capi.RRTX_OPT_NEAREST_REC_CAP, cap)


def _nearest_all_ways(ctx, pts, Q, meta, label, nqs=M.NQS):
    idx, dist, s = M.nearest_reference(pts, Q, meta["wraps"], meta["periods"])
    for nq in nqs:
        for mode in MODES:
            _set_mode(ctx, mode, nq, len(pts), len(meta["wraps"]))
            gi, gd = ctx.nn_nearest(Q[:nq])
            bad = np.flatnonzero((gi != idx[:nq]) | (_bits(gd) != _bits(dist[:nq])))
            assert len(bad) == 0, (f"{label}, {nq} queries, {mode}: query {bad[0]} has node {gi[bad[0]]} at "
                                   f"{gd[bad[0]]!r}, the reference node {idx[bad[0]]} at {dist[bad[0]]!r} "
                                   f"({len(bad)} differ)")
    return idx, dist, s


@pytest.mark.parametrize("name", sorted(SCENES))
def test_nearest_on_every_scene(oracle, name):
    pts, Q, meta = SCENES[name]()
    with _context(pts, meta) as ctx:
        idx, dist, s = _nearest_all_ways(ctx, pts, Q, meta, name)
    # the reference against the oracle: the distance bit for bit; the node too, or one at that same exact distance
    tree = oracle.KDTree(meta["dim"], list(meta["wraps"]), list(meta["periods"]))
    tree.insert_many(pts)
    for i in range(0, len(Q), 16):
        oi, od = tree.nearest(Q[i]) if meta["wraps"] else tree.nearest(Q[i], naive=True)
        assert od == dist[i] and s[i, oi] == s[i, idx[i]] and idx[i] <= oi, (name, i)


@functools.lru_cache(maxsize=None)
def _placement_scenes():
    return (("blind D3", M.blind(*M.BLIND[0], 3)), ("blind D4", M.blind(*M.BLIND[0], 4)), ("lattice D3", M.lattice(3)))


@pytest.mark.parametrize("n", [8, 9, 15])
def test_nearest_small_trees(n):
    """one group of 8 and no tail; 9 and 15: one group and a ragged tail in which every node is a candidate"""
    for label, scene in _placement_scenes():
        pts, Q, meta = M.placed(scene, n, "head")
        with _context(pts, meta) as ctx:
            _nearest_all_ways(ctx, pts, Q, meta, f"{label}, {n} nodes")


@pytest.mark.parametrize("n,placement", [(n, p) for n in M.SIZES if n > 15 for p in M.PLACEMENTS
                                         if p != "boundary" or M.nearest_segments(n, M.NQ)[0] > 1])
def test_nearest_cluster_positions(n, placement):
    """the cluster at the head of the node arrays (inside the warm start), across the boundary of two segments, and at
    the tail -- a ragged one for n % 8 = 1 and 7 -- among far nodes that are never the nearest"""
    for label, scene in _placement_scenes():
        pts, Q, meta = M.placed(scene, n, placement)
        with _context(pts, meta) as ctx:
            idx, _, _ = _nearest_all_ways(ctx, pts, Q, meta, f"{label}, {n} nodes, cluster at the {placement}",
                                          nqs=(50, 257) if n == 2100 else (1, 64))
        assert np.isin(idx, meta["cluster"]).all()


@pytest.mark.parametrize("D", [3, 4])
def test_nearest_between_and_after_two_appends(D):
    """the second append moves absmax, and with it C and M, while the fp32 shadow of the first part stays"""
    a, b, Q, meta = M.two_appends(M.blind(*M.BLIND[0], D))
    both = np.vstack([a, b])
    with _context(a, meta) as ctx:
        _nearest_all_ways(ctx, a, Q, meta, f"D{D}, first append", nqs=(64, 257))
        assert ctx.nodes_append(b) == len(a)
        idx, _, _ = _nearest_all_ways(ctx, both, Q, meta, f"D{D}, both appends", nqs=(64, 257))
    assert (idx >= len(a)).any() and (idx < len(a)).any()


@pytest.mark.parametrize("D", [3, 4])
def test_nearest_dev_form(D):
    """rrtx_nn_nearest_dev has no host round trip: the same answers from device buffers, on the stream"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    pts, Q, meta = M.blind(*M.BLIND[0], D)
    idx, dist, _ = M.nearest_reference(pts, Q)
    nq = len(Q)
    with _context(pts, meta) as ctx:
        d_q = torch.from_numpy(Q).to(dev)
        for mode in MODES:
            _set_mode(ctx, mode, nq, len(pts), 0)
            d_ni = torch.full((nq + 8,), -9, dtype=torch.int32, device=dev)
            d_nd = torch.full((nq + 8,), -9.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            ctx.nn_nearest_dev(d_q.data_ptr(), nq, d_ni.data_ptr(), d_nd.data_ptr())
            ctx.sync()
            gi, gd = d_ni.cpu().numpy(), d_nd.cpu().numpy()
            assert np.array_equal(gi[:nq], idx) and np.array_equal(_bits(gd[:nq]), _bits(dist)), mode
            assert (gi[nq:] == -9).all() and (gd[nq:] == -9.0).all()


# ---- range search -------------------------------------------------------------------------------------------------------
def _shell_scene(name):
    if name == "wrapped":
        return M.wrapped_shells()
    if name == "D3 far query":
        return M.shells(3, 1.0, far_query=True)
    return M.shells(4, float(name.split()[1]))


@pytest.mark.parametrize("name", ["D4 1", "D4 1e3", "D4 1e6", "wrapped", "D3 far query"])
def test_radius_shells(oracle, name):
    """nodes at r (1 + rel), rel down to 1e-16, around every query (test_radius_prefilter_is_conservative's
    construction) in D = 4 at three scales, around the ghosts of a wrapped D = 4 space, and in D = 3 with one query at
    1e7 that makes the shared C huge while the culled search keeps a C per copy: screen on and off, the culled search
    forced (2), at its default (1: off at this size) and off (0) -- the same lists, order and stored distances"""
    pts, Q, meta = _shell_scene(name)
    r = meta["r"]
    ref = M.range_reference(pts, Q, r, meta["wraps"], meta["periods"])
    tree = oracle.TreeSet(meta["dim"], pts, wraps=list(meta["wraps"]), wrap_points=list(meta["periods"]))
    orc = oracle.range_batch(tree, Q, r, nearest=False)
    assert np.array_equal(orc["offsets"], ref["offsets"]) and np.array_equal(orc["idx"], ref["idx"])
    assert np.array_equal(_bits(orc["key"]), _bits(ref["key"]))
    with _context(pts, meta) as ctx:
        for flt in (1, 0):
            for cull in (2, 1, 0):
                ctx.set_option(_capi.RRTX_OPT_NN_FILTER, flt)
                ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
                offsets, idx, dist = ctx.nn_radius(Q, r)
                label = f"shells {name}, filter {flt}, cull {cull}"
                assert np.array_equal(offsets, ref["offsets"]), f"{label}: list lengths differ"
                assert np.array_equal(idx, ref["idx"]), f"{label}: neighbour sets differ"
                assert np.array_equal(_bits(dist), _bits(ref["key"])), f"{label}: stored keys differ (bit-exact required)"
    if name in ("D4 1", "D3 far query"):
        assert int(np.sum(np.abs(ref["key"] - r) < 1e-12)) > 100        # the boundary cases really are exercised
    if name == "wrapped":
        assert int((ref["slot"] > 0).sum()) > 500


@pytest.mark.parametrize("name", sorted(SCENES))
def test_radius_through_the_clusters(name):
    """the range search on the cluster scenes themselves, the radius at twice the 90 % quantile of the nearest
    distances and at the cluster's half-width: the threshold cuts through nodes that fp32 cannot tell apart"""
    pts, Q, meta = SCENES[name]()
    _, dist, _ = M.nearest_reference(pts, Q, meta["wraps"], meta["periods"])
    with _context(pts, meta) as ctx:
        for r in (2.0 * float(np.quantile(dist, 0.9)), meta["rho"]):
            ref = M.range_reference(pts, Q, r, meta["wraps"], meta["periods"])
            assert len(ref["idx"]) >= 4 * len(Q)
            for flt, cull in ((1, 2), (1, 0), (0, 0)):
                ctx.set_option(_capi.RRTX_OPT_NN_FILTER, flt)
                ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
                offsets, idx, key = ctx.nn_radius(Q, r, cap=len(ref["idx"]) + 64)
                label = f"{name}, r = {r!r}, filter {flt}, cull {cull}"
                assert np.array_equal(offsets, ref["offsets"]), f"{label}: list lengths differ"
                assert np.array_equal(idx, ref["idx"]), f"{label}: neighbour sets differ"
                assert np.array_equal(_bits(key), _bits(ref["key"])), f"{label}: stored keys differ"


# ---- k nearest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(SCENES) if n.endswith("D3") and n.split()[0] in ("blind", "lattice")])
def test_knearest_rows(name):
    """rows by (distance, index) on the blind and lattice scenes, from the range lists (the culled search forced, so
    that 257 queries do take the list path and inherit the range screen) and from the exhaustive kernel"""
    pts, Q, meta = SCENES[name]()
    with _context(pts, meta) as ctx:
        for k in (1, 2, 8, 64, 65):
            ri, rd, rc = M.knearest_reference(pts, Q, k)
            for lists, cull in ((1, 2), (1, 1), (0, 1)):
                ctx.set_option(_capi.RRTX_OPT_KNN_LISTS, lists)
                ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
                gi, gd, gc = ctx.nn_knearest(Q, k)
                label = f"{name}, k = {k}, lists {lists}, cull {cull}"
                assert np.array_equal(gc, rc), label
                bad = np.argwhere((gi != ri) | (_bits(gd) != _bits(rd)))
                assert len(bad) == 0, (f"{label}: row {bad[0][0]} slot {bad[0][1]} has node {gi[tuple(bad[0])]} at "
                                       f"{gd[tuple(bad[0])]!r}, the reference {ri[tuple(bad[0])]} at "
                                       f"{rd[tuple(bad[0])]!r} ({len(bad)} differ)")


# ---- closest-self rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blind", "lattice"])
def test_closest_self_rows(oracle, kind):
    """the batch is the cluster: tau, the running k-th distance, tightens while t is inverted, so a thr' that lacks its
    K eps C^2 drops a true k-th neighbour here -- in the batch of 1000, the one with more than one tile of 512 earlier
    samples: the screen record follows tau once a tile, so up to 512 samples nothing is dropped at all.  Index, cost,
    count and both flag columns."""
    tree, samples, sphere, rr = M.closest_batch(kind)
    ref = E.closest_reference(oracle, samples, E.MAX_K, oracle.make_spheres(sphere), robot_radius=rr)
    hits = int(ref["hit_out"].sum())
    assert 0 < hits < int((ref["idx"] >= 0).sum()) and 0 < int(ref["hit_in"].sum())
    with Context(3) as ctx:
        ctx.nodes_append(tree)
        ctx.spheres_set(sphere)
        for b in M.CLOSEST_B:
            for k in M.CLOSEST_K:
                got, want = ctx.extend_closest_self(samples[:b], k, rr), E.narrow(ref, b, k)
                for f in E.FIELDS:
                    x, y = np.asarray(got[f]), np.asarray(want[f])
                    assert x.shape == y.shape and x.dtype == y.dtype, (kind, b, k, f)
                    if f == "cost":
                        x, y = _bits(x), _bits(y)
                    bad = np.argwhere(x != y)
                    assert len(bad) == 0, (f"{kind} batch of {b}, k = {k}, {f}{tuple(bad[0])}: {got[f][tuple(bad[0])]!r} "
                                           f"on the device, {want[f][tuple(bad[0])]!r} in the reference ({len(bad)} differ)")
