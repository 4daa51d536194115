"""The host-pointer extend calls against their own _dev forms: same context, same inputs, the host form into numpy arrays
and the _dev form into torch buffers, every returned array compared as bytes (NaN patterns included).  What is held to the
oracle is the _dev forms' business (test_gpu_extend_self*.py, test_gpu_extend_closest*.py, test_gpu_parity.py); here it is
the host layer: the device layout of the lists, the per-sample blocks, the staging arena and the direct route, the
capacity refusal, outputs that are not asked for, and the hold of rrtx_extend_select[_dubins].

rrtx_extend_candidates_dubins has no case here: its host form is not on the shared path."""
import ctypes as C

import numpy as np
import pytest

import extend_self_dubins_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR, RMIN = M.RR, M.RMIN
SENT, PAD = 0xA5, 5                     # every destination is PAD rows longer than it has to be, pre-filled with SENT bytes
I4, I8, F8, U1 = np.int32, np.int64, np.float64, np.uint8
CSR = ("candidates", "candidates_self", "candidates_self_dubins")
CLOSEST = ("closest_self", "closest_self_dubins")
R3, R4 = 1.5, 2.0


class Host:
    """destinations in pageable numpy arrays, the host form"""
    suffix = ""

    def alloc(self, shape, dtype):
        a = np.empty(shape, dtype=dtype)
        a.view(U1)[...] = SENT
        return a

    def up(self, a):
        return a

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def get(self, a):
        return a

    def ready(self):
        pass

    def needed(self):
        self._needed = C.c_int64(-1)
        return C.byref(self._needed)

    def needed_value(self):
        return int(self._needed.value)


class Dev:
    """destinations in torch buffers, the _dev form"""
    suffix = "_dev"

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", 0)

    def alloc(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return (self.torch.full((max(n, 1),), SENT, dtype=self.torch.uint8, device=self.dev), shape, dtype)

    def up(self, a):
        return None if a is None else (self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev), a.shape, a.dtype)

    def ptr(self, a):
        return None if a is None else a[0].data_ptr()

    def get(self, a):
        t, shape, dtype = a
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return t.cpu().numpy()[:n].view(dtype).reshape(shape)

    def ready(self):
        self.torch.cuda.synchronize()        # (the buffers are filled on torch's stream, the call runs on the context's)

    def needed(self):
        self._needed = self.alloc((1,), I8)
        return self.ptr(self._needed)

    def needed_value(self):
        return int(self.get(self._needed)[0])


def _run(ctx, mem, name, Q, *, r=None, k=None, cap=None, skip=None, want=None, tree_idx=None, drop=(), register=False):
    """one call of rrtx_extend_<name>[_dev]; returns (rc, {field: array with its PAD rows, or None if not passed})"""
    dub, closest, nq = name.endswith("dubins"), name in CLOSEST, len(Q)
    rows = nq * k if closest else cap
    o = {}

    def out(f, n, dtype, inner=(), on=True):
        o[f] = mem.alloc((n + PAD,) + inner, dtype) if on and f not in drop else None
        return mem.ptr(o[f])
    ins = [mem.up(x) for x in (Q, skip, want, tree_idx)]
    lists = [out("idx", rows, I4)] + [out(f, rows, F8) for f in (("key", "cost_out", "cost_in") if dub else ("cost",))]
    if dub:
        lists += [out("word_out", rows, U1, (3,)), out("word_in", rows, U1, (3,))]
    lists += [out("hit_out", rows, U1), out("hit_in", rows, U1)]
    head = [ctx.handle, mem.ptr(ins[0]), nq, k if closest else r, RR] + ([RMIN] if dub else [])
    if closest:
        tree = tree_idx is not None
        tail = [out("count", nq, I4)]
        if dub:
            tail += [out("tree_cost_out", nq, F8, on=tree), out("tree_cost_in", nq, F8, on=tree),
                     out("tree_word_out", nq, U1, (3,), on=tree), out("tree_word_in", nq, U1, (3,), on=tree)]
        tail += [out("tree_hit_out", nq, U1, on=tree), out("tree_hit_in", nq, U1, on=tree)]
        args = head + [mem.ptr(x) for x in ins[1:]] + lists + tail
    else:
        args = head + ([mem.ptr(ins[1])] if "self" in name else []) + [out("offsets", nq + 1, I8)] + lists + [cap, mem.needed()]
        if name == "candidates":
            args += [out("nearest_idx", nq, I4), out("nearest_dist", nq, F8), out("sample_unsafe", nq, U1)]
    if register:
        for a in o.values():
            ctx.host_register(a)
    mem.ready()
    rc = getattr(ctx._lib, "rrtx_extend_" + name + mem.suffix)(*args)
    ctx.sync()
    if register:
        for a in o.values():
            ctx.host_unregister(a)
    res = {f: (None if a is None else mem.get(a)) for f, a in o.items()}
    if not closest:
        res["needed"] = mem.needed_value()
    return rc, res


def _rows(name, f, nq, k, total):
    """rows of field f a call has to write"""
    if f == "offsets":
        return nq + 1
    if f in ("nearest_idx", "nearest_dist", "sample_unsafe", "count") or f.startswith("tree_"):
        return nq
    return nq * k if name in CLOSEST else total


def _same(name, a, b, nq, k=None, total=None, fields=None):
    """a and b agree byte for byte on what the call writes, and neither touched a byte beyond it"""
    for f in (fields or [f for f in a if f != "needed"]):
        x, y = a[f], b[f]
        assert (x is None) == (y is None), f
        if x is None:
            continue
        n = _rows(name, f, nq, k, total)
        assert x[:n].tobytes() == y[:n].tobytes(), f"{name}.{f} differs"
        assert (x[n:].view(U1) == SENT).all() and (y[n:].view(U1) == SENT).all(), f"{name}.{f}: bytes beyond row {n} written"


@pytest.fixture(scope="module")
def ctx3():
    rng = np.random.default_rng(31)
    sph = np.concatenate([rng.uniform(-5, 5, (12, 3)), rng.uniform(0.3, 1.0, (12, 1))], axis=1)
    with Context(3) as ctx:
        ctx.nodes_append(rng.uniform(-5, 5, (400, 3)))
        ctx.spheres_set(sph)
        yield ctx


def _ctx4(wraps):
    polys, kinds, paths = M.polygon_args("small", "flat")
    ctx = Context(4)
    for dim, period in zip(*wraps):
        ctx.set_wrap(dim, period)
    ctx.nodes_append(M.tree_points(300, 3.0))
    ctx.polygons_set(polys, kinds=kinds, paths=paths)
    return ctx


@pytest.fixture(scope="module")
def ctx4():
    with _ctx4(M.THETA) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def ctx4_flat():
    with _ctx4(((), ())) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("torch")
    return Dev()


def _samples(dim, nq, seed=32):
    if dim == 4:
        return np.ascontiguousarray(M.random_samples("small")[:nq]) if nq <= 65 else None
    return np.random.default_rng(seed).uniform(-5, 5, (nq, 3))


def _total(ctx, dev, name, Q, r, skip=None):
    """the entry count, by the _dev form with no room at all"""
    rc, out = _run(ctx, dev, name, Q, r=r, cap=0, skip=skip, drop=("idx", "cost", "key", "cost_out", "cost_in", "word_out",
                                                                   "word_in", "hit_out", "hit_in"))
    assert rc == _capi.RRTX_OK
    return out["needed"]


def _pick(name, ctx3, ctx4):
    return (ctx4, 4, R4) if name.endswith("dubins") else (ctx3, 3, R3)


@pytest.mark.parametrize("nq", [1, 2, 65])
@pytest.mark.parametrize("name", CSR)
def test_csr_calls_equal_their_dev_forms(ctx3, ctx4, dev, name, nq):
    ctx, dim, r = _pick(name, ctx3, ctx4)
    Q = _samples(dim, nq)
    total = _total(ctx, dev, name, Q, r)
    rc_d, ref = _run(ctx, dev, name, Q, r=r, cap=total)
    rc_h, got = _run(ctx, Host(), name, Q, r=r, cap=total)                      # cap == total exactly
    assert rc_d == rc_h == _capi.RRTX_OK and got["needed"] == ref["needed"] == total
    _same(name, got, ref, nq, total=total)
    if nq == 65:
        assert total > 0
        rc, reg = _run(ctx, Host(), name, Q, r=r, cap=total, register=True)     # every destination by direct DMA
        assert rc == _capi.RRTX_OK
        _same(name, reg, ref, nq, total=total)
        rc, short = _run(ctx, Host(), name, Q, r=r, cap=total - 1)
        assert rc == _capi.RRTX_E_CAPACITY and short["needed"] == total
        assert short["offsets"].tobytes() == got["offsets"].tobytes()
        per_entry = [f for f in short if f not in ("offsets", "needed", "nearest_idx", "nearest_dist", "sample_unsafe")]
        assert all((short[f].view(U1) == SENT).all() for f in per_entry)
    rc, none = _run(ctx, Host(), name, Q, r=r, cap=0, drop=("idx", "cost", "key", "cost_out", "cost_in", "word_out", "word_in",
                                                            "hit_out", "hit_in"))
    assert rc == (_capi.RRTX_E_CAPACITY if total else _capi.RRTX_OK) and none["needed"] == total
    assert none["offsets"].tobytes() == got["offsets"].tobytes()


@pytest.mark.parametrize("name", CSR)
def test_a_batch_with_empty_lists(ctx3, ctx4, dev, name):
    ctx, dim, _ = _pick(name, ctx3, ctx4)
    Q = _samples(dim, 65)
    r = 1e-9
    rc_d, ref = _run(ctx, dev, name, Q, r=r, cap=4)
    rc_h, got = _run(ctx, Host(), name, Q, r=r, cap=4)
    assert rc_d == rc_h == _capi.RRTX_OK and got["needed"] == ref["needed"] == 0 and not got["offsets"][:66].any()
    _same(name, got, ref, 65, total=0)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nq", [1, 2, 65])
@pytest.mark.parametrize("name", CLOSEST)
def test_closest_calls_equal_their_dev_forms(ctx3, ctx4, ctx4_flat, dev, name, nq, k):
    for ctx in ((ctx4, ctx4_flat) if name.endswith("dubins") else (ctx3,)):
        Q = _samples(ctx.dim, nq)
        rng = np.random.default_rng(33)
        skip, want = (rng.random(nq) < 0.2).astype(U1), (rng.random(nq) < 0.7).astype(U1)
        tree_idx = rng.integers(-1, ctx.n_nodes, nq).astype(I4)
        for kw in (dict(), dict(skip=skip), dict(want=want), dict(tree_idx=tree_idx), dict(skip=skip, want=want, tree_idx=tree_idx)):
            rc_d, ref = _run(ctx, dev, name, Q, k=k, **kw)
            rc_h, got = _run(ctx, Host(), name, Q, k=k, **kw)
            assert rc_d == rc_h == _capi.RRTX_OK
            _same(name, got, ref, nq, k=k)
        if nq == 65:
            rc, reg = _run(ctx, Host(), name, Q, k=k, register=True, skip=skip, want=want, tree_idx=tree_idx)
            assert rc == _capi.RRTX_OK
            _same(name, reg, ref, nq, k=k)


def test_outputs_not_asked_for(ctx3, ctx4, dev):
    Q3, Q4 = _samples(3, 65), _samples(4, 65)
    skip = (np.random.default_rng(34).random(65) < 0.2).astype(U1)
    tree_idx = np.random.default_rng(35).integers(0, 300, 65).astype(I4)
    cases = [("candidates", ctx3, Q3, dict(r=R3), [("nearest_idx",), ("nearest_dist",), ("nearest_idx", "nearest_dist"),
                                                   ("sample_unsafe",)]),
             ("candidates_self", ctx3, Q3, dict(r=R3, skip=skip), []),
             ("candidates_self_dubins", ctx4, Q4, dict(r=R4, skip=skip), [("word_out", "word_in"), ("word_out",)]),
             ("closest_self_dubins", ctx4, Q4, dict(k=3, tree_idx=tree_idx),
              [("word_out", "word_in"), ("tree_word_out", "tree_word_in"), ("word_in", "tree_word_out")])]
    for name, ctx, Q, kw, drops in cases:
        if "k" not in kw:
            kw["cap"] = _total(ctx, dev, name, Q, kw["r"], kw.get("skip"))
        rc, full = _run(ctx, Host(), name, Q, **kw)
        assert rc == _capi.RRTX_OK
        if "skip" in kw and "k" not in kw:                   # skip present against skip absent: other lists
            rc, ref = _run(ctx, dev, name, Q, **kw)
            _same(name, full, ref, 65, total=kw["cap"])
        for drop in drops:
            rc, part = _run(ctx, Host(), name, Q, drop=drop, **kw)
            assert rc == _capi.RRTX_OK and all(part[f] is None for f in drop)
            # (nearest_idx without nearest_dist, or the reverse: neither is written)
            unwritten = ("nearest_idx", "nearest_dist") if set(drop) & {"nearest_idx", "nearest_dist"} else ()
            rest = [f for f in part if f != "needed" and f not in drop and f not in unwritten]
            _same(name, part, full, 65, k=kw.get("k"), total=kw.get("cap"), fields=rest)
            assert all(part[f] is None or (part[f].view(U1) == SENT).all() for f in unwritten)


def _big_3d():
    rng = np.random.default_rng(36)
    return rng.uniform(-5, 5, (2000, 3)), 2.6


def _big_4d():
    return np.ascontiguousarray(M.random_samples("large")), 4.4


@pytest.mark.parametrize("space", [3, 4])
def test_lists_whose_double_columns_go_direct(ctx3, ctx4, dev, space):
    """between 32 769 and 65 536 entries a double column is above 256 KB and goes straight to the caller while idx and the
    flag bytes are staged"""
    name, ctx, (Q, r) = ("candidates", ctx3, _big_3d()) if space == 3 else ("candidates_self_dubins", ctx4, _big_4d())
    total = _total(ctx, dev, name, Q, r)
    assert 32769 <= total <= 65536, total
    rc_d, ref = _run(ctx, dev, name, Q, r=r, cap=total)
    rc_h, got = _run(ctx, Host(), name, Q, r=r, cap=total)
    assert rc_d == rc_h == _capi.RRTX_OK
    _same(name, got, ref, len(Q), total=total)


def _mirror(ctx):
    return [a.tobytes() for a in ctx.graph_edges_get()]


@pytest.mark.parametrize("dubins", [False, True])
def test_hold(ctx3, ctx4, dubins):
    ctx, dim, r = (ctx4, 4, R4) if dubins else (ctx3, 3, R3)
    Q = _samples(dim, 65)
    lmc = np.random.default_rng(37).uniform(0.0, 10.0, ctx.n_nodes)
    select = (lambda: ctx.extend_select_dubins(Q, r, RR, RMIN, lmc=lmc, want_lists=True)) if dubins else \
             (lambda: ctx.extend_select(Q, r, RR, lmc=lmc, want_lists=True))
    node_of = np.full(65, -1, dtype=I4)
    node_of[::2] = np.arange(33) % ctx.n_nodes
    # directly after a select the held lists are linked: the mirror append_lists makes of the same lists
    sel = select()
    ctx.graph_edges_clear()
    first, added, rows = ctx.graph_edges_append_selected(node_of)
    held = _mirror(ctx)
    ctx.graph_edges_clear()
    cols = ("offsets", "idx", "cost_out", "cost_in", "hit_out", "hit_in") if dubins else ("offsets", "idx", "cost", "cost", "hit_out", "hit_in")
    first_b, added_b, rows_b = ctx.graph_edges_append_lists(*[sel[c] for c in cols], node_of)
    assert added == added_b > 0 and np.array_equal(rows, rows_b) and held == _mirror(ctx)
    ctx.graph_edges_clear()
    # every host call of the family drops the hold
    for name in [n for n in CSR + CLOSEST if n.endswith("dubins") == dubins]:
        select()
        rc, _ = _run(ctx, Host(), name, Q, r=r, k=1, cap=0, drop=("idx", "cost", "key", "cost_out", "cost_in", "word_out",
                                                                  "word_in", "hit_out", "hit_in") if name in CSR else ())
        assert rc in (_capi.RRTX_OK, _capi.RRTX_E_CAPACITY)
        f, a = C.c_int64(), C.c_int64()
        rc = ctx._lib.rrtx_graph_edges_append_selected(ctx.handle, 65, _capi._ptr(node_of), C.byref(f), C.byref(a), None)
        assert rc == _capi.RRTX_E_STATE, name
        assert ctx.n_graph_edges == 0
