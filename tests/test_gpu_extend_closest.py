"""rrtx_extend_closest_self -- the k nearest earlier samples of an extend batch, for the closestNode rule -- against the
reference of tests/extend_closest_model.py (held to the oracle's kdFindNearest in tests/test_extend_closest_scenes.py).
Every comparison is bit for bit: idx, the costs as bit patterns, both flag arrays, the counts, the tree column."""
import numpy as np
import pytest

import extend_closest_model as M
import extend_self_model as S
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR = M.RR
KS = (1, 2, 8, 32)


def _same(got, ref, fields=M.FIELDS, label=""):
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{label}{f}: {a.shape} {a.dtype} on the device, {b.shape} {b.dtype}"
        if f == "cost":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (f"{label}{f}{tuple(bad[0])}: {got[f][tuple(bad[0])]!r} on the device, "
                               f"{ref[f][tuple(bad[0])]!r} in the reference ({len(bad)} differ)")


def _context(kind, name, tree=None):
    ctx = Context(3)
    if tree is not None:
        ctx.nodes_append(tree)
    if kind == "spheres":
        ctx.spheres_set(S.lattice_spheres() if name == "lattice" else S.random_spheres(name))
    else:
        ctx.polygons_set(S.random_polygons(name))
        ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
    return ctx


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
@pytest.mark.parametrize("b", sorted(S.SIZES))
def test_random_scenes(oracle, kind, b):
    """the single row and the batch of two, the wave's and the workgroup's edges (63 / 64 / 65 rows: a group of rows is
    16), 257 rows and a second tile of columns at 1000; every k at which a row is shorter than, exactly, and longer than
    the list; a context with obstacles and no tree"""
    name = S.SIZES[b]
    Q, ref = M.scene(kind, name)
    with _context(kind, name) as ctx:
        for k in KS:
            _same(ctx.extend_closest_self(Q[:b], k, RR), M.narrow(ref, b, k), label=f"k = {k}: ")


@pytest.mark.parametrize("k", KS)
def test_lattice_scene(oracle, k):
    """ties on s at the k-th place (the lower index stays), pairs at distance 0 (which collide with every sphere)"""
    Q, ref = M.scene("spheres", "lattice")
    with _context("spheres", "lattice") as ctx:
        got = ctx.extend_closest_self(Q, k, RR)
        _same(got, M.narrow(ref, len(Q), k))
        assert ((got["cost"] == 0.0) & (got["idx"] >= 0)).sum() >= 3


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_want(oracle, kind):
    """want NULL is every live row; all zero fills nothing and disturbs nothing else; a random half fills its rows with
    what they hold when all are wanted: a sample that is not wanted is still a candidate of the others"""
    Q, ref = M.scene(kind, "large")
    ref = M.narrow(ref, len(Q), 8)
    obs = S.obstacles(oracle, kind, "large")
    with _context(kind, "large") as ctx:
        none = ctx.extend_closest_self(Q, 8, RR, want=np.zeros(len(Q), dtype=np.uint8))
        assert (none["count"] == 0).all() and (none["idx"] == -1).all() and (none["cost"] == np.inf).all()
        assert not none["hit_out"].any() and not none["hit_in"].any()
        _same(ctx.extend_closest_self(Q, 8, RR, want=np.ones(len(Q), dtype=np.uint8)), ref)
        want = (np.random.default_rng(3).random(len(Q)) < 0.5).astype(np.uint8)
        half = ctx.extend_closest_self(Q, 8, RR, want=want)
        _same(half, M.closest_reference(oracle, Q, 8, obs, want=want))
        assert (want[half["idx"][half["idx"] >= 0]] == 0).any()
        # a single wanted row at the end of the batch, and one at its beginning
        for j in (len(Q) - 1, 0):
            one = np.zeros(len(Q), dtype=np.uint8)
            one[j] = 1
            _same(ctx.extend_closest_self(Q, 8, RR, want=one), M.closest_reference(oracle, Q, 8, obs, want=one))


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_skip_and_non_finite_samples(oracle, kind):
    Q, skip = M.marked_samples()
    obs = S.obstacles(oracle, kind, "mid")
    with _context(kind, "mid") as ctx:
        got = ctx.extend_closest_self(Q, 8, RR, skip=skip)
        _same(got, M.closest_reference(oracle, Q, 8, obs, skip=skip))
        for j in (M.MARKED, M.NOT_FINITE):
            assert got["count"][j] == 0 and not (got["idx"] == j).any()
        # every kind of non-finite coordinate, a third of the samples marked, and want on top
        bad = S.random_samples("large").copy()
        bad[10, 0], bad[200, 2], bad[201, 1] = np.nan, np.inf, -np.inf
        skip = (np.random.default_rng(6).random(len(bad)) < 1.0 / 3.0).astype(np.uint8)
        want = (np.random.default_rng(7).random(len(bad)) < 0.5).astype(np.uint8)
    obs = S.obstacles(oracle, kind, "large")
    with _context(kind, "large") as ctx:
        _same(ctx.extend_closest_self(bad, 8, RR, skip=skip), M.closest_reference(oracle, bad, 8, obs, skip=skip))
        _same(ctx.extend_closest_self(bad, 2, RR, skip=skip, want=want),
              M.closest_reference(oracle, bad, 2, obs, skip=skip, want=want))


def test_huge_coordinates_switch_the_screen_off(oracle):
    """a live sample far outside the fp32 range: C is huge, the screen drops nothing, and s overflows for its pairs,
    which are then in no row"""
    Q = S.random_samples("mid").copy()
    Q[40] = [1.0e200, 0.0, 0.0]
    Q[41] = [1.0e17, 1.0, 1.0]
    obs = S.obstacles(oracle, "spheres", "mid")
    ref = M.closest_reference(oracle, Q, 8, obs)
    assert not (ref["idx"] == 40).any() and ref["count"][40] == 0 and ref["count"][41] == 8
    with _context("spheres", "mid") as ctx:
        _same(ctx.extend_closest_self(Q, 8, RR), ref)


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_tree_column(oracle, kind):
    Q = S.random_samples("mid")
    tree = S.tree_points(200, S.RANDOM["mid"][1])
    obs = S.obstacles(oracle, kind, "mid")
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    ti[5], ti[6], ti[7] = -1, len(tree), 2 ** 31 - 1
    want = (np.random.default_rng(9).random(len(Q)) < 0.5).astype(np.uint8)
    fields = M.FIELDS + M.TREE_FIELDS
    with _context(kind, "mid", tree) as ctx:
        got = ctx.extend_closest_self(Q, 2, RR, tree_idx=ti)
        ref = M.closest_reference(oracle, Q, 2, obs, tree_idx=ti, tree_pts=tree)
        _same(got, ref, fields)
        assert 0 < ref["tree_hit_out"].sum() < len(Q)
        # only the filled rows have a tree column
        got = ctx.extend_closest_self(Q, 2, RR, want=want, tree_idx=ti)
        _same(got, M.closest_reference(oracle, Q, 2, obs, want=want, tree_idx=ti, tree_pts=tree), fields)
        assert not got["tree_hit_out"][want == 0].any() and not got["tree_hit_in"][want == 0].any()
        # the nearest node of the extend call on the same batch, as it is
        cand = ctx.extend_candidates(Q, S.RANDOM["mid"][2], RR)
        got = ctx.extend_closest_self(Q, 8, RR, skip=cand["sample_unsafe"], tree_idx=cand["nearest_idx"])
        _same(got, M.closest_reference(oracle, Q, 8, obs, skip=cand["sample_unsafe"], tree_idx=cand["nearest_idx"],
                                       tree_pts=tree), fields)
    # an empty tree: every index is out of range, the rows are the rows
    with _context(kind, "mid") as ctx:
        got = ctx.extend_closest_self(Q, 2, RR, tree_idx=ti)
        _same(got, M.closest_reference(oracle, Q, 2, obs, tree_idx=ti, tree_pts=None), fields)
        assert not got["tree_hit_out"].any() and not got["tree_hit_in"].any()


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_flags_are_those_of_edges_check(kind):
    """byte for byte what rrtx_edges_check returns for the directed edge"""
    Q = S.random_samples("large")
    with _context(kind, "large") as ctx:
        got = ctx.extend_closest_self(Q, 8, RR)
        j, slot = np.nonzero(got["idx"] >= 0)
        i = got["idx"][j, slot]
        k = 1 if kind == "polygons" else 0
        out, _ = ctx.edges_check(Q[j], Q[i], RR, kind=k)
        back, _ = ctx.edges_check(Q[i], Q[j], RR, kind=k)
        assert np.array_equal(got["hit_out"][j, slot], out.astype(np.uint8))
        assert np.array_equal(got["hit_in"][j, slot], back.astype(np.uint8))


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_dev_form(oracle, kind):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    Q, ref = M.scene(kind, "large")
    nq, k = len(Q), 8
    tree = S.tree_points(200)
    obs = S.obstacles(oracle, kind, "large")
    skip = (np.random.default_rng(6).random(nq) < 0.1).astype(np.uint8)
    want = (np.random.default_rng(7).random(nq) < 0.5).astype(np.uint8)
    ti = np.random.default_rng(8).integers(-1, len(tree) + 1, nq).astype(np.int32)
    with _context(kind, "large", tree) as ctx:
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_q, d_skip = torch.from_numpy(Q).to(dev), torch.from_numpy(skip).to(dev)
            d_want, d_ti = torch.from_numpy(want).to(dev), torch.from_numpy(ti).to(dev)
            # a guard row behind every array: nothing at or past nq * k (nq) is touched
            d_idx = torch.full((nq + 1, k), -7, dtype=torch.int32, device=dev)
            d_cost = torch.full((nq + 1, k), -7.0, dtype=torch.float64, device=dev)
            d_ho = torch.full((nq + 1, k), 77, dtype=torch.uint8, device=dev)
            d_hi = torch.full((nq + 1, k), 77, dtype=torch.uint8, device=dev)
            d_cnt = torch.full((nq + 8,), -7, dtype=torch.int32, device=dev)
            d_tho = torch.full((nq + 8,), 77, dtype=torch.uint8, device=dev)
            d_thi = torch.full((nq + 8,), 77, dtype=torch.uint8, device=dev)
            st.synchronize()

            def run(skip_ptr, want_ptr, tree):
                ctx.extend_closest_self_dev(d_q.data_ptr(), nq, k, RR, skip_ptr, want_ptr, d_ti.data_ptr() if tree else None,
                                            d_idx.data_ptr(), d_cost.data_ptr(), d_ho.data_ptr(), d_hi.data_ptr(),
                                            d_cnt.data_ptr(), d_tho.data_ptr() if tree else None,
                                            d_thi.data_ptr() if tree else None)
                st.synchronize()
                full = dict(idx=d_idx.cpu().numpy(), cost=d_cost.cpu().numpy(), hit_out=d_ho.cpu().numpy(),
                            hit_in=d_hi.cpu().numpy(), count=d_cnt.cpu().numpy(), tree_hit_out=d_tho.cpu().numpy(),
                            tree_hit_in=d_thi.cpu().numpy())
                assert (full["idx"][nq:] == -7).all() and (full["cost"][nq:] == -7.0).all()
                assert (full["hit_out"][nq:] == 77).all() and (full["hit_in"][nq:] == 77).all()
                assert (full["count"][nq:] == -7).all()
                assert (full["tree_hit_out"][nq if tree else 0:] == 77).all()
                assert (full["tree_hit_in"][nq if tree else 0:] == 77).all()
                return {f: v[:nq] for f, v in full.items()}
            _same(run(None, None, False), M.narrow(ref, nq, k))
            _same(run(d_skip.data_ptr(), d_want.data_ptr(), True),
                  M.closest_reference(oracle, Q, k, obs, skip=skip, want=want, tree_idx=ti, tree_pts=tree),
                  M.FIELDS + M.TREE_FIELDS)
        ctx.set_stream(None)
        # the host form on the same context, after the device form
        _same(ctx.extend_closest_self(Q, k, RR), M.narrow(ref, nq, k))


def _code(ctx, dim, k, nq=8, tree=(True, True, True)):
    n, kk = max(nq, 1), max(k, 1)
    q = np.random.default_rng(9).uniform(-3.0, 3.0, (n, dim))
    idx, cost = np.empty((n, kk), dtype=np.int32), np.empty((n, kk))
    ho, hi = np.empty((n, kk), dtype=np.uint8), np.empty((n, kk), dtype=np.uint8)
    cnt, ti = np.empty(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    tho, thi = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
    p = _capi._ptr
    return ctx._lib.rrtx_extend_closest_self(ctx.handle, p(q), nq, k, RR, None, None, p(ti) if tree[0] else None, p(idx),
                                             p(cost), p(ho), p(hi), p(cnt), p(tho) if tree[1] else None,
                                             p(thi) if tree[2] else None)


def test_refused_inputs():
    with Context(3) as ctx:
        ctx.nodes_append(np.random.default_rng(1).uniform(-3, 3, (50, 3)))
        ctx.spheres_set(S.random_spheres("small"))
        assert _capi.RRTX_CLOSEST_SELF_MAX_K == 32
        assert _code(ctx, 3, 8) == _capi.RRTX_OK and _code(ctx, 3, 1) == _capi.RRTX_OK and _code(ctx, 3, 32) == _capi.RRTX_OK
        assert _code(ctx, 3, 8, tree=(False, False, False)) == _capi.RRTX_OK
        assert _code(ctx, 3, 8, nq=0) == _capi.RRTX_OK
        for k in (0, 33, -1):
            assert _code(ctx, 3, k) == _capi.RRTX_E_INVALID, k
        assert _code(ctx, 3, 8, nq=-1) == _capi.RRTX_E_INVALID
        for tree in ((True, False, False), (False, True, True), (True, True, False)):
            assert _code(ctx, 3, 8, tree=tree) == _capi.RRTX_E_INVALID, tree
        with pytest.raises(RrtxError):
            ctx.extend_closest_self(np.zeros((4, 3)), 0, RR)
        ctx.set_wrap(0, 6.0)
        assert _code(ctx, 3, 8) == _capi.RRTX_E_STATE
    with Context(4) as ctx:
        ctx.nodes_append(np.random.default_rng(1).uniform(-3, 3, (50, 4)))
        assert _code(ctx, 4, 8) == _capi.RRTX_E_STATE
