"""rrtx_extend_candidates_self_dubins -- the samples of one Dubins extend batch among themselves, in the wrapped space --
against the oracle-side reference of tests/extend_self_dubins_model.py (held to an all-pairs restatement of the ghost
rule in tests/test_extend_self_dubins_scenes.py).  Every comparison is ==: offsets, idx, the keys and costs as bit
patterns, the words and both flag arrays."""
import ctypes as C

import numpy as np
import pytest

import extend_self_dubins_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR, RMIN = M.RR, M.RMIN
FIELDS = ("offsets", "idx", "key", "cost_out", "cost_in", "word_out", "word_in", "hit_out", "hit_in")


def _same(got, ref, label="", fields=FIELDS):
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, f"{label}{k}: {a.shape} on the device, {b.shape} in the reference"
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{label}{k}[{bad[0]}]: {got[k][bad[0]]!r} on the device, {ref[k][bad[0]]!r} in the reference"


def _context(name, mode="flat", tree=None):
    _, _, (polys, kinds, paths), wraps = M.scene_inputs(name, mode)
    ctx = Context(4)
    for dim, period in zip(*wraps):
        ctx.set_wrap(dim, period)
    if tree is not None:
        ctx.nodes_append(tree)
    ctx.polygons_set(polys, kinds=kinds, paths=paths)
    opt = M.MODES[mode]
    if opt["has_time"]:
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(opt["v_min"], opt["v_max"])
        ctx.set_dubins_time_column(_capi.RRTX_TIME_COLUMN_PIECEWISE if opt["piecewise"]
                                   else _capi.RRTX_TIME_COLUMN_RUNNING_SUM)
    return ctx


@pytest.mark.parametrize("b", sorted(M.SIZES))
def test_flat_scenes(oracle, b):
    """theta wrapped, no time: the wave and row-group edges of the join (63 / 64 / 65 rows), more rows than the threads
    of a tile load (257), two tiles of columns and several workgroups (1000), the single row and the batch of two"""
    name = M.SIZES[b]
    Q, ref = M.scene(name)
    with _context(name) as ctx:
        _same(ctx.extend_candidates_self_dubins(Q[:b], M.RANDOM[name][2], RR, RMIN), M.prefix(ref, b))


@pytest.mark.parametrize("mode", ["time", "moving"])
@pytest.mark.parametrize("b", sorted(M.TIME_SIZES))
def test_scenes_with_time(oracle, b, mode):
    """RRTX_OPT_SPACE_HAS_TIME with velocities set (bit 1 of a flag byte = !validMove); "moving": polygons that move
    along paths and the running-sum time column"""
    name = M.TIME_SIZES[b]
    Q, ref = M.scene(name, mode)
    with _context(name, mode) as ctx:
        got = ctx.extend_candidates_self_dubins(Q[:b], M.RANDOM[name][2], RR, RMIN)
        _same(got, M.prefix(ref, b))
        assert set(got["hit_out"].tolist()) | set(got["hit_in"].tolist()) == {0, 1, 2, 3}


def test_no_two_columns_can_be_transposed(oracle):
    """65 samples, theta wrapped, one static and one moving polygon, time on: on the oracle's answer alone cost_out /
    cost_in, word_out / word_in and hit_out / hit_in each differ in at least a quarter of the entries, so a call that
    hands two columns of a pair out in each other's place cannot equal it"""
    Q, r = M.random_samples("small"), M.RANDOM["small"][2]
    polys, kinds, paths = M.two_polygons()
    ref = M.self_reference(oracle, Q, r, oracle.PolygonSet(polys, kinds=kinds, paths=paths), "moving")
    pairs = (("cost_out", "cost_in"), ("word_out", "word_in"), ("hit_out", "hit_in"))
    share = M.transposed_share(ref, np.ones(len(ref["idx"]), dtype=bool), pairs)
    assert len(ref["idx"]) >= 65 and min(share.values()) >= 0.25, share
    with _context("small", "moving") as ctx:
        ctx.polygons_set(polys, kinds=kinds, paths=paths)
        got = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN)
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), f


@pytest.mark.parametrize("r", M.LATTICE_R)
def test_lattice_scenes(oracle, r):
    """pairs at distance exactly r are no neighbours; duplicates are neighbours at key 0"""
    Q, ref = M.scene("lattice", "flat", r)
    with _context("lattice") as ctx:
        got = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN, cap=16)          # (grows on demand)
        _same(got, ref)
        assert (got["key"] == 0.0).sum() >= 3


@pytest.mark.parametrize("name", sorted(M.TWO_WRAPS) + ["nowrap"])
def test_two_wraps_and_none(oracle, name):
    """four copies of a sample in either order of rrtx_set_wrap, and a space without a wrapped dimension"""
    Q, ref = M.scene(name)
    with _context(name) as ctx:
        _same(ctx.extend_candidates_self_dubins(Q, M.RANDOM["mid"][2], RR, RMIN), ref)


def _merge(cand, self_, n0):
    """the tree list of every sample, then its batch list with idx + n0: the node every earlier sample receives when
    all of them are inserted"""
    ca, sa = np.diff(cand["offsets"]), np.diff(self_["offsets"])
    offsets = np.zeros(len(ca) + 1, dtype=np.int64)
    np.cumsum(ca + sa, out=offsets[1:])
    out = dict(offsets=offsets)
    for k in FIELDS[1:]:
        a, b = cand[k], (self_[k] + n0 if k == "idx" else self_[k])
        rows = [np.concatenate([a[cand["offsets"][j]:cand["offsets"][j + 1]], b[self_["offsets"][j]:self_["offsets"][j + 1]]])
                for j in range(len(ca))]
        out[k] = np.concatenate(rows).astype(a.dtype)
    return out


def test_union_with_the_tree_lists_is_the_reference_list(oracle):
    tree, Q, r = M.tree_points(), M.random_samples("large"), M.RANDOM["large"][2]
    polys, kinds, paths = M.polygon_args("large", "flat")
    ref = M.merged_reference(oracle, tree, Q, r, oracle.PolygonSet(polys, kinds=kinds, paths=paths))
    with _context("large", tree=tree) as ctx:
        cand = ctx.extend_candidates_dubins(Q, r, RR, RMIN)
        self_ = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN)
        assert len(cand["idx"]) > 0 and len(self_["idx"]) > 0
        _same(_merge(cand, self_, len(tree)), ref)
        # the tree is not read: the same lists as from a context without one
        _same(self_, M.scene("large")[1])


def test_skip(oracle):
    Q, r = M.random_samples("large"), M.RANDOM["large"][2]
    polys, kinds, paths = M.polygon_args("large", "flat")
    ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths)
    skip = (np.random.default_rng(6).random(len(Q)) < 1.0 / 3.0).astype(np.uint8)
    with _context("large", tree=M.tree_points()) as ctx:
        got = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN, skip=skip)
        _same(got, M.self_reference(oracle, Q, r, ps, skip=skip))
        assert (np.diff(got["offsets"])[skip != 0] == 0).all() and not skip[got["idx"]].any()
        # the sample_unsafe bytes of the extend call on the same batch, as they are
        unsafe = ctx.extend_candidates_dubins(Q, r, RR, RMIN)["sample_unsafe"]
        assert unsafe.dtype == np.uint8 and 0 < unsafe.sum() < len(Q)
        _same(ctx.extend_candidates_self_dubins(Q, r, RR, RMIN, skip=unsafe), M.self_reference(oracle, Q, r, ps, skip=unsafe))


@pytest.mark.parametrize("col", range(4))
def test_non_finite_samples(col):
    Q, r = M.random_samples("large"), M.RANDOM["large"][2]
    bad = Q.copy()
    bad[10, col] = np.nan
    bad[200, col] = np.inf
    bad[700, col] = -np.inf
    skip = np.zeros(len(Q), dtype=np.uint8)
    skip[[10, 200, 700]] = 1
    with _context("large") as ctx:
        got = ctx.extend_candidates_self_dubins(bad, r, RR, RMIN)
        counts = np.diff(got["offsets"])
        assert (counts[[10, 200, 700]] == 0).all() and not np.isin(got["idx"], [10, 200, 700]).any()
        assert len(got["idx"]) > 5000
        _same(got, ctx.extend_candidates_self_dubins(Q, r, RR, RMIN, skip=skip))


def _raw(ctx, Q, r, cap, arrays=True, words=True):
    nq = len(Q)
    n = max(cap, 1)
    offsets = np.full(nq + 1, -1, dtype=np.int64)
    idx = np.full(n, -7, dtype=np.int32)
    key, co, ci = np.full(n, -7.0), np.full(n, -7.0), np.full(n, -7.0)
    wo, wi = np.full((n, 3), 77, dtype=np.uint8), np.full((n, 3), 77, dtype=np.uint8)
    ho, hi = np.full(n, 77, dtype=np.uint8), np.full(n, 77, dtype=np.uint8)
    needed = C.c_int64(-1)
    p = (lambda a: _capi._ptr(a)) if arrays else (lambda a: None)
    w = p if words else (lambda a: None)
    rc = ctx._lib.rrtx_extend_candidates_self_dubins(ctx.handle, _capi._ptr(Q) if nq else None, nq, r, RR, RMIN, None,
                                                     _capi._ptr(offsets), p(idx), p(key), p(co), p(ci), w(wo), w(wi), p(ho),
                                                     p(hi), cap, C.byref(needed))
    out = dict(offsets=offsets, idx=idx, key=key, cost_out=co, cost_in=ci, word_out=wo.view("S3").ravel(),
               word_in=wi.view("S3").ravel(), hit_out=ho, hit_in=hi)
    return rc, int(needed.value), out


def test_capacity(oracle):
    Q, ref = M.scene("mid")
    r, n = M.RANDOM["mid"][2], len(ref["idx"])
    with _context("mid") as ctx:
        rc, needed, out = _raw(ctx, Q, r, n - 1)
        assert rc == _capi.RRTX_E_CAPACITY and needed == n and np.array_equal(out["offsets"], ref["offsets"])
        assert (out["idx"] == -7).all() and (out["key"] == -7.0).all() and (out["hit_out"] == 77).all()   # nothing written
        rc, needed, out = _raw(ctx, Q, r, 0, arrays=False)                      # cap == 0 with NULL arrays counts
        assert rc == _capi.RRTX_E_CAPACITY and needed == n and np.array_equal(out["offsets"], ref["offsets"])
        rc, needed, out = _raw(ctx, Q[:1], r, 0, arrays=False)                  # ... and nothing to count is no error
        assert rc == _capi.RRTX_OK and needed == 0 and np.array_equal(out["offsets"], [0, 0])
        rc, needed, out = _raw(ctx, Q[:0], r, 0, arrays=False)                  # nq == 0
        assert rc == _capi.RRTX_OK and needed == 0 and out["offsets"][0] == 0
        rc, needed, out = _raw(ctx, Q, r, n)                                    # exactly enough
        assert rc == _capi.RRTX_OK and needed == n
        _same(out, ref)


def test_words_may_be_null(oracle):
    Q, ref = M.scene("mid")
    r, n = M.RANDOM["mid"][2], len(ref["idx"])
    with _context("mid") as ctx:
        rc, needed, out = _raw(ctx, Q, r, n, words=False)
        assert rc == _capi.RRTX_OK and needed == n
        _same(out, ref, fields=[f for f in FIELDS if not f.startswith("word")])
        assert (out["word_out"] == b"MMM").all() and (out["word_in"] == b"MMM").all()        # (77: untouched)


def test_radius_that_reaches_nothing():
    Q = M.random_samples("mid")
    with _context("mid") as ctx:
        for r in (0.0, -1.0, float("nan")):
            rc, needed, out = _raw(ctx, Q, r, 8)
            assert rc == _capi.RRTX_OK and needed == 0 and not out["offsets"].any()


def test_dev_form(oracle):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    Q, ref = M.scene("large")
    nq, r, n = len(Q), M.RANDOM["large"][2], len(ref["idx"])
    skip = (np.random.default_rng(6).random(nq) < 0.1).astype(np.uint8)
    with _context("large") as ctx:
        host = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN)
        host_skip = ctx.extend_candidates_self_dubins(Q, r, RR, RMIN, skip=skip)
        _same(host, ref)
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            cap = n + 5
            d_q, d_skip = torch.from_numpy(Q).to(dev), torch.from_numpy(skip).to(dev)
            d_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
            d_idx = torch.full((cap,), -7, dtype=torch.int32, device=dev)
            d_f = {k: torch.full((cap,), -7.0, dtype=torch.float64, device=dev) for k in ("key", "cost_out", "cost_in")}
            d_w = {k: torch.full((cap, 3), 77, dtype=torch.uint8, device=dev) for k in ("word_out", "word_in")}
            d_h = {k: torch.full((cap,), 77, dtype=torch.uint8, device=dev) for k in ("hit_out", "hit_in")}
            d_need = torch.zeros(1, dtype=torch.int64, device=dev)
            st.synchronize()

            def run(skip_ptr, cap, words=True):
                ctx.extend_candidates_self_dubins_dev(
                    d_q.data_ptr(), nq, r, RR, RMIN, skip_ptr, d_off.data_ptr(), d_idx.data_ptr(), d_f["key"].data_ptr(),
                    d_f["cost_out"].data_ptr(), d_f["cost_in"].data_ptr(), d_w["word_out"].data_ptr() if words else None,
                    d_w["word_in"].data_ptr() if words else None, d_h["hit_out"].data_ptr(), d_h["hit_in"].data_ptr(), cap,
                    d_need.data_ptr())
                st.synchronize()
                got = dict(offsets=d_off.cpu().numpy(), idx=d_idx.cpu().numpy())
                got.update({k: v.cpu().numpy() for k, v in d_f.items()})
                got.update({k: v.cpu().numpy().view("S3").ravel() for k, v in d_w.items()})
                got.update({k: v.cpu().numpy() for k, v in d_h.items()})
                return int(d_need.item()), got

            def untouched(got, a):
                return ((got["idx"][a:] == -7).all() and all((got[k][a:] == -7.0).all() for k in d_f)
                        and all((got[k][a:] == b"MMM").all() for k in d_w) and all((got[k][a:] == 77).all() for k in d_h))
            k, got = run(None, cap)
            assert k == n
            _same({f: (got[f] if f == "offsets" else got[f][:k]) for f in FIELDS}, host)
            assert untouched(got, k)                           # nothing at or past the count is touched
            k, got = run(d_skip.data_ptr(), cap)
            _same({f: (got[f] if f == "offsets" else got[f][:k]) for f in FIELDS}, host_skip)
            # a short capacity: the count and the offsets are right, nothing is written at or past cap
            fills = [(d_idx, -7)] + [(t, -7.0) for t in d_f.values()] + [(t, 77) for t in list(d_w.values()) + list(d_h.values())]
            for t, v in fills:
                t.fill_(v)
            st.synchronize()
            short = n // 2
            k, got = run(None, short)
            assert k == n and np.array_equal(got["offsets"], ref["offsets"]) and untouched(got, short)
            # the words are optional
            for t in d_w.values():
                t.fill_(77)
            st.synchronize()
            k, got = run(None, cap, words=False)
            rest = [f for f in FIELDS if not f.startswith("word")]
            assert k == n and all((got[f] == b"MMM").all() for f in d_w)
            _same({f: (got[f] if f == "offsets" else got[f][:k]) for f in rest}, host, fields=rest)
        ctx.set_stream(None)


def test_refused_inputs():
    """a dim-3 context is RRTX_E_STATE, as for rrtx_extend_candidates_dubins; negative counts and NULL arrays with
    cap > 0 are RRTX_E_INVALID"""
    p = _capi._ptr
    q = np.random.default_rng(9).uniform(0.0, 3.0, (8, 4))
    cap = 256
    off = np.zeros(9, dtype=np.int64)
    idx, f = np.empty(cap, dtype=np.int32), [np.empty(cap) for _ in range(3)]
    h = [np.empty(cap, dtype=np.uint8) for _ in range(2)]
    needed = C.c_int64(-1)

    def call(ctx, nq=8, cap=cap, q_=q, off_=off, idx_=idx, key=f[0], ho=h[0]):
        return ctx._lib.rrtx_extend_candidates_self_dubins(ctx.handle, p(q_), nq, 2.0, RR, RMIN, None, p(off_), p(idx_),
                                                           p(key), p(f[1]), p(f[2]), None, None, p(ho), p(h[1]), cap,
                                                           C.byref(needed))
    with Context(3) as ctx:
        ctx.nodes_append(np.random.default_rng(1).uniform(-3, 3, (50, 3)))
        assert call(ctx) == _capi.RRTX_E_STATE
    with _context("mid") as ctx:
        assert call(ctx) == _capi.RRTX_OK                   # no tree: still a call
        assert call(ctx, nq=-1) == _capi.RRTX_E_INVALID
        assert call(ctx, cap=-1) == _capi.RRTX_E_INVALID
        assert call(ctx, q_=None) == _capi.RRTX_E_INVALID
        assert call(ctx, off_=None) == _capi.RRTX_E_INVALID
        assert call(ctx, idx_=None) == _capi.RRTX_E_INVALID
        assert call(ctx, key=None) == _capi.RRTX_E_INVALID
        assert call(ctx, ho=None) == _capi.RRTX_E_INVALID
        assert call(ctx, cap=0, idx_=None, key=None, ho=None) in (_capi.RRTX_OK, _capi.RRTX_E_CAPACITY)
