"""rrtx_extend_closest_self_dubins -- the k nearest earlier samples of a Dubins extend batch in the wrapped space, for the
closestNode rule -- against the reference of tests/extend_closest_dubins_model.py (held to the oracle's kdFindNearest in
tests/test_extend_closest_dubins_scenes.py).  Every comparison is ==: idx, the keys and costs as bit patterns, the words,
both flag arrays, the counts, the tree column."""
import numpy as np
import pytest

import extend_closest_dubins_model as M
import extend_self_dubins_model as S
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR, RMIN = M.RR, M.RMIN
KS = (1, 2, 8, 32)
ALL = M.FIELDS + M.TREE_FIELDS


def _same(got, ref, fields=M.FIELDS, label=""):
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{label}{f}: {a.shape} {a.dtype} on the device, {b.shape} {b.dtype}"
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (f"{label}{f}{tuple(bad[0])}: {got[f][tuple(bad[0])]!r} on the device, "
                               f"{ref[f][tuple(bad[0])]!r} in the reference ({len(bad)} differ)")


def _context(name, mode="flat", tree=None):
    _, (polys, kinds, paths), wraps = M.scene_inputs(name, mode)
    ctx = Context(4)
    for dim, period in zip(*wraps):
        ctx.set_wrap(dim, period)
    if tree is not None:
        ctx.nodes_append(tree)
    ctx.polygons_set(polys, kinds=kinds, paths=paths)
    opt = S.MODES[mode]
    if opt["has_time"]:
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(opt["v_min"], opt["v_max"])
        ctx.set_dubins_time_column(_capi.RRTX_TIME_COLUMN_PIECEWISE if opt["piecewise"]
                                   else _capi.RRTX_TIME_COLUMN_RUNNING_SUM)
    return ctx


@pytest.mark.parametrize("b", sorted(S.SIZES))
def test_flat_scenes(oracle, b):
    """theta wrapped: the single row and the batch of two, the wave's and the workgroup's edges (63 / 64 / 65 rows: a
    group of rows is 4), 257 rows and a second tile of columns at 1000; every k at which a row is shorter than, exactly,
    and longer than the list; a context with obstacles and no tree"""
    name = S.SIZES[b]
    Q, ref, _ = M.scene(name)
    with _context(name) as ctx:
        for k in KS:
            _same(ctx.extend_closest_self_dubins(Q[:b], k, RR, RMIN), M.narrow(ref, b, k), label=f"k = {k}: ")


@pytest.mark.parametrize("name", ["nowrap", "theta_t", "t_theta", "three"])
@pytest.mark.parametrize("b", [65, 257])
def test_other_wraps(oracle, name, b):
    """one, four (either order of rrtx_set_wrap) and eight copies of a sample through the same kernel"""
    Q, ref, _ = M.scene(name)
    with _context(name) as ctx:
        for k in KS:
            _same(ctx.extend_closest_self_dubins(Q[:b], k, RR, RMIN), M.narrow(ref, b, k), label=f"k = {k}: ")


@pytest.mark.parametrize("mode", ["time", "moving"])
@pytest.mark.parametrize("b", sorted(S.TIME_SIZES))
def test_scenes_with_time(oracle, b, mode):
    """RRTX_OPT_SPACE_HAS_TIME with velocities set (bit 1 of a flag byte = !validMove); "moving": polygons that move
    along paths and the running-sum time column"""
    name = S.TIME_SIZES[b]
    Q, ref, _ = M.scene(name, mode)
    with _context(name, mode) as ctx:
        for k in (2, 8):
            got = ctx.extend_closest_self_dubins(Q[:b], k, RR, RMIN)
            _same(got, M.narrow(ref, b, k), label=f"k = {k}: ")
        assert set(got["hit_out"].ravel().tolist()) | set(got["hit_in"].ravel().tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("k", KS)
def test_lattice_scene(oracle, k):
    """ties on s at the k-th place (the lower index stays), pairs at distance 0"""
    Q, ref, _ = M.scene("lattice")
    with _context("lattice") as ctx:
        got = ctx.extend_closest_self_dubins(Q, k, RR, RMIN)
        _same(got, M.narrow(ref, len(Q), k))
        assert ((got["key"] == 0.0) & (got["idx"] >= 0)).sum() >= 3


def test_want(oracle):
    """want NULL is every live row; all zero fills nothing and disturbs nothing else; a random half fills its rows with
    what they hold when all are wanted: a sample that is not wanted is still a candidate of the others"""
    Q, ref, _ = M.scene("large")
    ref = M.narrow(ref, len(Q), 8)
    ps = M.polygon_set(oracle, "large")
    with _context("large") as ctx:
        none = ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, want=np.zeros(len(Q), dtype=np.uint8))
        assert (none["count"] == 0).all() and (none["idx"] == -1).all() and (none["key"] == np.inf).all()
        assert (none["cost_out"] == np.inf).all() and (none["cost_in"] == np.inf).all()
        assert (none["word_out"] == M.NO_WORD).all() and (none["word_in"] == M.NO_WORD).all()
        assert not none["hit_out"].any() and not none["hit_in"].any()
        _same(ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, want=np.ones(len(Q), dtype=np.uint8)), ref)
        want = (np.random.default_rng(3).random(len(Q)) < 0.5).astype(np.uint8)
        half = ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, want=want)
        _same(half, M.closest_reference(oracle, Q, 8, ps, want=want))
        assert (want[half["idx"][half["idx"] >= 0]] == 0).any()
        # a single wanted row at the end of the batch, and one at its beginning
        for j in (len(Q) - 1, 0):
            one = np.zeros(len(Q), dtype=np.uint8)
            one[j] = 1
            _same(ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, want=one), M.closest_reference(oracle, Q, 8, ps, want=one))


def test_skip_and_non_finite_samples(oracle):
    Q, skip = M.marked_samples()
    ps = M.polygon_set(oracle, "mid")
    with _context("mid") as ctx:
        got = ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, skip=skip)
        _same(got, M.closest_reference(oracle, Q, 8, ps, skip=skip))
        for j in (M.MARKED, M.NOT_FINITE):
            assert got["count"][j] == 0 and not (got["idx"] == j).any()
    # every kind of non-finite value in each of the four coordinates, a third of the samples marked, and want on top
    ps = M.polygon_set(oracle, "large")
    skip = (np.random.default_rng(6).random(1000) < 1.0 / 3.0).astype(np.uint8)
    want = (np.random.default_rng(7).random(1000) < 0.5).astype(np.uint8)
    with _context("large") as ctx:
        for col in range(4):
            bad = S.random_samples("large").copy()
            bad[10, col], bad[200, col], bad[201, col] = np.nan, np.inf, -np.inf
            _same(ctx.extend_closest_self_dubins(bad, 8, RR, RMIN), M.closest_reference(oracle, bad, 8, ps),
                  label=f"column {col}: ")
        _same(ctx.extend_closest_self_dubins(bad, 8, RR, RMIN, skip=skip), M.closest_reference(oracle, bad, 8, ps, skip=skip))
        _same(ctx.extend_closest_self_dubins(bad, 2, RR, RMIN, skip=skip, want=want),
              M.closest_reference(oracle, bad, 2, ps, skip=skip, want=want))


def test_huge_coordinates_switch_the_screen_off(oracle):
    """a live sample far outside the fp32 range: C is huge, the screen drops nothing, and s overflows for its pairs,
    which are then in no row"""
    Q = S.random_samples("mid").copy()
    Q[40, 0] = 1.0e200
    ps = M.polygon_set(oracle, "mid")
    ref = M.closest_reference(oracle, Q, 8, ps)
    assert not (ref["idx"] == 40).any() and ref["count"][40] == 0 and ref["count"][41] == 8
    with _context("mid") as ctx:
        _same(ctx.extend_closest_self_dubins(Q, 8, RR, RMIN), ref)


def test_tree_column(oracle):
    Q = S.random_samples("mid")
    tree = S.tree_points(200, S.RANDOM["mid"][1])
    ps = M.polygon_set(oracle, "mid")
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    ti[5], ti[6], ti[7] = -1, len(tree), 2 ** 31 - 1
    want = (np.random.default_rng(9).random(len(Q)) < 0.5).astype(np.uint8)
    with _context("mid", tree=tree) as ctx:
        got = ctx.extend_closest_self_dubins(Q, 2, RR, RMIN, tree_idx=ti)
        ref = M.closest_reference(oracle, Q, 2, ps, tree_idx=ti, tree_pts=tree)
        _same(got, ref, ALL)
        assert 0 < ref["tree_hit_out"].sum() < len(Q)
        # only the filled rows have a tree column
        got = ctx.extend_closest_self_dubins(Q, 2, RR, RMIN, want=want, tree_idx=ti)
        _same(got, M.closest_reference(oracle, Q, 2, ps, want=want, tree_idx=ti, tree_pts=tree), ALL)
        assert not got["tree_hit_out"][want == 0].any() and (got["tree_cost_in"][want == 0] == np.inf).all()
        # the nearest node of the extend call on the same batch, as it is
        cand = ctx.extend_candidates_dubins(Q, S.RANDOM["mid"][2], RR, RMIN)
        got = ctx.extend_closest_self_dubins(Q, 8, RR, RMIN, skip=cand["sample_unsafe"], tree_idx=cand["nearest_idx"])
        _same(got, M.closest_reference(oracle, Q, 8, ps, skip=cand["sample_unsafe"], tree_idx=cand["nearest_idx"],
                                       tree_pts=tree), ALL)
    # an empty tree: every index is out of range, the rows are the rows
    with _context("mid") as ctx:
        got = ctx.extend_closest_self_dubins(Q, 2, RR, RMIN, tree_idx=ti)
        _same(got, M.closest_reference(oracle, Q, 2, ps, tree_idx=ti, tree_pts=None), ALL)
        assert not got["tree_hit_out"].any() and (got["tree_cost_out"] == np.inf).all()


def test_tree_column_with_time(oracle):
    Q = S.random_samples("small")
    tree = S.tree_points(100, S.RANDOM["small"][1])
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    with _context("small", "moving", tree=tree) as ctx:
        ref = M.closest_reference(oracle, Q, 2, M.polygon_set(oracle, "small", "moving"), "moving", tree_idx=ti,
                                  tree_pts=tree)
        _same(ctx.extend_closest_self_dubins(Q, 2, RR, RMIN, tree_idx=ti), ref, ALL)
        assert len(set(ref["tree_hit_out"].tolist())) >= 3


def test_no_two_columns_can_be_transposed(oracle):
    """65 samples over a tree of 257 nodes, k = 3, theta wrapped, one static and one moving polygon, time on: on the
    oracle's answer alone cost_out / cost_in, word_out / word_in and hit_out / hit_in each differ in at least a quarter
    of the used slots, and so do the three pairs of the tree column over the filled rows, so a call that hands two
    columns of a pair out in each other's place cannot equal it"""
    Q = S.random_samples("small")
    tree = S.tree_points(257, S.RANDOM["small"][1])
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    polys, kinds, paths = S.two_polygons()
    ref = M.closest_reference(oracle, Q, 3, oracle.PolygonSet(polys, kinds=kinds, paths=paths), "moving", tree_idx=ti,
                              tree_pts=tree)
    pairs = (("cost_out", "cost_in"), ("word_out", "word_in"), ("hit_out", "hit_in"))
    share = S.transposed_share(ref, ref["idx"] >= 0, pairs)
    share.update(S.transposed_share(ref, ref["count"] > 0, [("tree_" + a, "tree_" + b) for a, b in pairs]))
    assert (ref["idx"] >= 0).sum() >= 65 and min(share.values()) >= 0.25, share
    with _context("small", "moving", tree=tree) as ctx:
        ctx.polygons_set(polys, kinds=kinds, paths=paths)
        got = ctx.extend_closest_self_dubins(Q, 3, RR, RMIN, tree_idx=ti)
    for f in ALL:
        assert np.array_equal(got[f], ref[f]), f


@pytest.mark.parametrize("mode", ["flat", "time"])
def test_entries_are_those_of_dubins_edges_check(mode):
    """byte for byte and bit for bit what rrtx_dubins_edges_check returns for the directed edge; with time bit 1 of a
    flag byte is !validMove of rrtx_dubins_steer_full"""
    Q = S.random_samples("mid")
    with _context("mid", mode) as ctx:
        got = ctx.extend_closest_self_dubins(Q, 8, RR, RMIN)
        j, slot = np.nonzero(got["idx"] >= 0)
        i = got["idx"][j, slot]
        for a, b, d in ((j, i, "out"), (i, j, "in")):
            cost, word, hit, _ = ctx.dubins_edges_check(Q[a], Q[b], RMIN, RR)
            bad = 0
            if mode == "time":
                bad = 2 * (ctx.dubins_steer_full(Q[a], Q[b], RMIN)["valid_move"] == 0).astype(np.uint8)
            assert np.array_equal(got["cost_" + d][j, slot].view(np.uint64), cost.view(np.uint64))
            assert np.array_equal(got["word_" + d][j, slot], word)
            assert np.array_equal(got["hit_" + d][j, slot], hit.astype(np.uint8) | bad)


def _raw(ctx, Q, k, words=True, tree=None):
    """the C entry point with every output filled beforehand: (return code, dict)"""
    nq = len(Q)
    p = _capi._ptr
    idx = np.full((nq, k), -7, dtype=np.int32)
    f = [np.full((nq, k), -7.0) for _ in range(3)]
    w = [np.full((nq, k, 3), 77, dtype=np.uint8) for _ in range(2)]
    h = [np.full((nq, k), 77, dtype=np.uint8) for _ in range(2)]
    cnt = np.full(nq, -7, dtype=np.int32)
    tf = [np.full(nq, -7.0) for _ in range(2)]
    tw = [np.full((nq, 3), 77, dtype=np.uint8) for _ in range(2)]
    th = [np.full(nq, 77, dtype=np.uint8) for _ in range(2)]
    t = tree is not None
    rc = ctx._lib.rrtx_extend_closest_self_dubins(
        ctx.handle, p(Q), nq, k, RR, RMIN, None, None, p(tree) if t else None, p(idx), p(f[0]), p(f[1]), p(f[2]),
        p(w[0]) if words else None, p(w[1]) if words else None, p(h[0]), p(h[1]), p(cnt), p(tf[0]) if t else None,
        p(tf[1]) if t else None, p(tw[0]) if t and words else None, p(tw[1]) if t and words else None,
        p(th[0]) if t else None, p(th[1]) if t else None)
    return rc, dict(idx=idx, key=f[0], cost_out=f[1], cost_in=f[2], word_out=w[0].view("S3").reshape(nq, k),
                    word_in=w[1].view("S3").reshape(nq, k), hit_out=h[0], hit_in=h[1], count=cnt, tree_cost_out=tf[0],
                    tree_cost_in=tf[1], tree_word_out=tw[0].view("S3").reshape(nq), tree_word_in=tw[1].view("S3").reshape(nq),
                    tree_hit_out=th[0], tree_hit_in=th[1])


def test_words_may_be_null(oracle):
    Q = S.random_samples("mid")
    tree = S.tree_points(200, S.RANDOM["mid"][1])
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    ref = M.closest_reference(oracle, Q, 8, M.polygon_set(oracle, "mid"), tree_idx=ti, tree_pts=tree)
    rest = [f for f in ALL if "word" not in f]
    with _context("mid", tree=tree) as ctx:
        rc, out = _raw(ctx, Q, 8, words=False, tree=ti)
        assert rc == _capi.RRTX_OK
        _same(out, ref, rest)
        assert all((out[f] == b"MMM").all() for f in ALL if "word" in f)        # (77: untouched)
        rc, out = _raw(ctx, Q, 8, words=True, tree=ti)
        assert rc == _capi.RRTX_OK
        _same(out, ref, ALL)
        # without a tree column nothing of it is written
        rc, out = _raw(ctx, Q, 8)
        assert rc == _capi.RRTX_OK and (out["tree_cost_out"] == -7.0).all() and (out["tree_hit_in"] == 77).all()
        _same(out, ref)


def test_dev_form(oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    Q, ref, _ = M.scene("large")
    nq, k = len(Q), 8
    tree = S.tree_points(200)
    ps = M.polygon_set(oracle, "large")
    skip = (np.random.default_rng(6).random(nq) < 0.1).astype(np.uint8)
    want = (np.random.default_rng(7).random(nq) < 0.5).astype(np.uint8)
    ti = np.random.default_rng(8).integers(-1, len(tree) + 1, nq).astype(np.int32)
    with _context("large", tree=tree) as ctx:
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_q, d_skip = torch.from_numpy(Q).to(dev), torch.from_numpy(skip).to(dev)
            d_want, d_ti = torch.from_numpy(want).to(dev), torch.from_numpy(ti).to(dev)
            # guard rows in front of and behind every array: nothing outside [0, nq * k) (or [0, nq)) is touched
            g = 2

            def guarded(rows, cols, dtype, fill):
                return torch.full((rows + 2 * g,) + cols, fill, dtype=dtype, device=dev)
            rowf = {f: guarded(nq, (k,), torch.float64, -7.0) for f in ("key", "cost_out", "cost_in")}
            roww = {f: guarded(nq, (k, 3), torch.uint8, 77) for f in ("word_out", "word_in")}
            rowh = {f: guarded(nq, (k,), torch.uint8, 77) for f in ("hit_out", "hit_in")}
            d_idx = guarded(nq, (k,), torch.int32, -7)
            d_cnt = guarded(nq, (), torch.int32, -7)
            tf = {f: guarded(nq, (), torch.float64, -7.0) for f in ("tree_cost_out", "tree_cost_in")}
            tw = {f: guarded(nq, (3,), torch.uint8, 77) for f in ("tree_word_out", "tree_word_in")}
            th = {f: guarded(nq, (), torch.uint8, 77) for f in ("tree_hit_out", "tree_hit_in")}
            every = dict(idx=d_idx, count=d_cnt, **rowf, **roww, **rowh, **tf, **tw, **th)
            fills = {torch.float64: -7.0, torch.uint8: 77, torch.int32: -7}
            st.synchronize()

            def ptr(t, on=True):
                return t[g:].data_ptr() if on else None

            def run(skip_ptr, want_ptr, tree, words=True):
                for t in every.values():
                    t.fill_(fills[t.dtype])
                ctx.extend_closest_self_dubins_dev(
                    d_q.data_ptr(), nq, k, RR, RMIN, skip_ptr, want_ptr, d_ti.data_ptr() if tree else None, ptr(d_idx),
                    ptr(rowf["key"]), ptr(rowf["cost_out"]), ptr(rowf["cost_in"]), ptr(roww["word_out"], words),
                    ptr(roww["word_in"], words), ptr(rowh["hit_out"]), ptr(rowh["hit_in"]), ptr(d_cnt),
                    ptr(tf["tree_cost_out"], tree), ptr(tf["tree_cost_in"], tree), ptr(tw["tree_word_out"], tree and words),
                    ptr(tw["tree_word_in"], tree and words), ptr(th["tree_hit_out"], tree), ptr(th["tree_hit_in"], tree))
                st.synchronize()
                out = {}
                for f, t in every.items():
                    a = t.cpu().numpy()
                    written = not ((f.startswith("tree") and not tree) or ("word" in f and not words))
                    guard = np.concatenate([a[:g].ravel(), a[g + nq:].ravel()]) if written else a.ravel()
                    assert (guard == fills[t.dtype]).all(), f
                    a = a[g:g + nq]
                    out[f] = a.view("S3").reshape(a.shape[:-1]) if "word" in f else a
                return out
            _same(run(None, None, False), M.narrow(ref, nq, k))
            full = M.closest_reference(oracle, Q, k, ps, skip=skip, want=want, tree_idx=ti, tree_pts=tree)
            _same(run(d_skip.data_ptr(), d_want.data_ptr(), True), full, ALL)
            _same(run(d_skip.data_ptr(), d_want.data_ptr(), True, words=False), full, [f for f in ALL if "word" not in f])
        ctx.set_stream(None)
        # the host form on the same context, after the device form
        _same(ctx.extend_closest_self_dubins(Q, k, RR, RMIN), M.narrow(ref, nq, k))


def _code(ctx, dim, k, nq=8, tree=(True,) * 5, drop=None):
    n, kk = max(nq, 1), max(k, 1)
    q = np.random.default_rng(9).uniform(0.0, 3.0, (n, dim))
    a = dict(q=q, idx=np.empty((n, kk), dtype=np.int32), key=np.empty((n, kk)), cost_out=np.empty((n, kk)),
             cost_in=np.empty((n, kk)), hit_out=np.empty((n, kk), dtype=np.uint8), hit_in=np.empty((n, kk), dtype=np.uint8),
             count=np.empty(n, dtype=np.int32))
    t = [np.zeros(n, dtype=np.int32), np.empty(n), np.empty(n), np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)]
    t = [_capi._ptr(x) if on else None for x, on in zip(t, tree)]
    p = {f: (None if f == drop else _capi._ptr(v)) for f, v in a.items()}
    return ctx._lib.rrtx_extend_closest_self_dubins(ctx.handle, p["q"], nq, k, RR, RMIN, None, None, t[0], p["idx"], p["key"],
                                                    p["cost_out"], p["cost_in"], None, None, p["hit_out"], p["hit_in"],
                                                    p["count"], t[1], t[2], None, None, t[3], t[4])


def test_refused_inputs():
    with _context("small", tree=S.tree_points(50, 3.0)) as ctx:
        assert _code(ctx, 4, 8) == _capi.RRTX_OK and _code(ctx, 4, 1) == _capi.RRTX_OK and _code(ctx, 4, 32) == _capi.RRTX_OK
        assert _code(ctx, 4, 8, tree=(False,) * 5) == _capi.RRTX_OK
        assert _code(ctx, 4, 8, nq=0) == _capi.RRTX_OK
        for k in (0, 33, -1):
            assert _code(ctx, 4, k) == _capi.RRTX_E_INVALID, k
        assert _code(ctx, 4, 8, nq=-1) == _capi.RRTX_E_INVALID
        for n in range(5):
            assert _code(ctx, 4, 8, tree=tuple(m != n for m in range(5))) == _capi.RRTX_E_INVALID, n
            assert _code(ctx, 4, 8, tree=tuple(m == n for m in range(5))) == _capi.RRTX_E_INVALID, n
        for f in ("q", "idx", "key", "cost_out", "cost_in", "hit_out", "hit_in", "count"):
            assert _code(ctx, 4, 8, drop=f) == _capi.RRTX_E_INVALID, f
        with pytest.raises(RrtxError):
            ctx.extend_closest_self_dubins(np.zeros((4, 4)), 0, RR, RMIN)
    with Context(3) as ctx:
        ctx.nodes_append(np.random.default_rng(1).uniform(-3, 3, (50, 3)))
        assert _code(ctx, 3, 8) == _capi.RRTX_E_STATE
