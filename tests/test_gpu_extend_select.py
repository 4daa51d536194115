"""findBestParent and the rewire test of extend() on the device (rrtx_extend_select_dev, rrtx_extend_select,
rrtx_node_cost_set) against the numpy restatement of tests/test_select_reference.py applied to the lists the existing
host calls return.  Every comparison is np.array_equal over every sample and entry: each output is an input value, an
index or one rounded fp64 addition.  The conditions on the inputs (ties, statuses, non-empty rewire lists) are asserted
on the reference alone, so no test passes by being empty."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from rrtqx_3d_amd import _capi, drrt, synth
from rrtqx_3d_amd._capi import RrtxError
from rrtqx_3d_amd.context import Context

from test_select_reference import (KEYS, SEL_EMPTY, SEL_NO_PARENT, SEL_OK, SEL_OVERFLOW, SEL_UNSAFE, select_numpy,
                                   tie_samples)

pytestmark = pytest.mark.gpu
RR = 0.5
ROOT = os.path.dirname(os.path.abspath(__file__))


def _assert_same(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype, (what, k, got[k].dtype, ref[k].dtype)
        assert np.array_equal(got[k], ref[k]), (what, k)


def _scene_queries(cfg, sph):
    """The configuration's batch, with a few samples far outside the world (empty balls) and a few at obstacle
    centres (unsafe) in the place of its last ones."""
    Q = synth.queries(cfg.batch, 3).copy()
    Q[-8:] = np.array([400.0, -300.0, 250.0]) + np.arange(8)[:, None]
    Q[-16:-8] = sph[:8, :3] + 0.125
    return Q


def _random_lmc(n, seed):
    """Non-negative values, some orphans (+Inf), one NaN; the root at 0."""
    rng = np.random.default_rng(seed)
    lmc = rng.uniform(0.0, 60.0, n)
    lmc[rng.random(n) < 0.3] = math.inf
    lmc[0] = 0.0
    lmc[n // 2] = math.nan
    return lmc


def _mirror_random_tree(ctx, n, seed):
    """Every node but the root and a few orphans gets an edge to a random earlier node, plus some cross edges."""
    rng = np.random.default_rng(seed)
    child = np.arange(1, n)
    child = child[rng.random(n - 1) > 0.002]
    par = (rng.random(len(child)) * child).astype(np.int64)
    extra_s = rng.integers(1, n, n // 2)
    extra_e = (rng.random(n // 2) * extra_s).astype(np.int64)
    ctx.graph_edges_append(np.concatenate([child, extra_s]), np.concatenate([par, extra_e]))


class _Dev:
    """Device buffers for one extend -> select chain (torch tensors; pointers go through the C-ABI)."""

    def __init__(self, torch, nq, cap, rw_cap, dubins=False):
        dev = torch.device("cuda", 0)
        self.torch, self.nq, self.cap, self.rw_cap = torch, nq, cap, rw_cap
        t = lambda m, dt, fill: torch.full((max(m, 1),), fill, dtype=dt, device=dev)
        self.off = t(nq + 1, torch.int64, -7)
        self.idx = t(cap, torch.int32, -7)
        self.cost = t(cap, torch.float64, -7.0)
        self.cost_in = t(cap, torch.float64, -7.0) if dubins else self.cost
        self.key = t(cap, torch.float64, -7.0) if dubins else None
        self.ho, self.hi = t(cap, torch.uint8, 7), t(cap, torch.uint8, 7)
        self.need = t(1, torch.int64, -7)
        self.ni, self.nd, self.un = t(nq, torch.int32, -7), t(nq, torch.float64, -7.0), t(nq, torch.uint8, 7)
        self.pi, self.pe = t(nq, torch.int32, -7), t(nq, torch.int64, -7)
        self.ln, self.st = t(nq, torch.float64, -7.0), t(nq, torch.uint8, 77)
        self.rwo = t(nq + 1, torch.int64, -7)
        self.rwn, self.rwv = t(rw_cap, torch.int32, -7), t(rw_cap, torch.float64, -7.0)
        self.rwneed = t(1, torch.int64, -7)
        torch.cuda.synchronize()

    def select(self, ctx, lmc_ptr, unsafe=True, rw_cap=None, hit_out=None, n_valid=True, cap=None):
        ctx.extend_select_dev(self.nq, self.off.data_ptr(), self.idx.data_ptr(), self.cost.data_ptr(), self.cost_in.data_ptr(),
                              (self.ho if hit_out is None else hit_out).data_ptr(), self.hi.data_ptr(),
                              self.need.data_ptr() if n_valid else None, self.cap if cap is None else cap,
                              self.un.data_ptr() if unsafe else None, lmc_ptr, self.pi.data_ptr(), self.pe.data_ptr(),
                              self.ln.data_ptr(), self.st.data_ptr(), self.rwo.data_ptr(), self.rwn.data_ptr(),
                              self.rwv.data_ptr(), self.rw_cap if rw_cap is None else rw_cap, self.rwneed.data_ptr())
        ctx.sync()
        n = int(self.rwneed.item())
        h = lambda x: x.cpu().numpy()
        return dict(status=h(self.st)[:self.nq], parent_idx=h(self.pi)[:self.nq], parent_entry=h(self.pe)[:self.nq],
                    lmc_new=h(self.ln)[:self.nq], rw_offsets=h(self.rwo), rw_node=h(self.rwn)[:max(min(n, self.rw_cap), 0)],
                    rw_value=h(self.rwv)[:max(min(n, self.rw_cap), 0)], rw_needed=n)


def _extend_dev(ctx, d, Q, r):
    dq = d.torch.from_numpy(np.ascontiguousarray(Q)).to(d.off.device)
    ctx.extend_candidates_dev(dq.data_ptr(), d.nq, r, RR, d.off.data_ptr(), d.idx.data_ptr(), d.cost.data_ptr(),
                              d.ho.data_ptr(), d.hi.data_ptr(), d.cap, d.need.data_ptr(), d.ni.data_ptr(), d.nd.data_ptr(),
                              d.un.data_ptr())
    ctx.sync()


def _reference(lists, lmc, unsafe=True, cost_in="cost"):
    return select_numpy(lists["offsets"], lists["idx"], lists["cost_out" if "cost_out" in lists else "cost"],
                        lists[cost_in], lists["hit_out"], lists["hit_in"], lists["sample_unsafe"] if unsafe else None, lmc)


def _ok_share_with_rewire(ref):
    ok = ref["status"] == SEL_OK
    return (np.diff(ref["rw_offsets"])[ok] > 0).sum() / max(ok.sum(), 1)


# ---- C2 and C4 size, device form -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,lmc_kind", [("C2", "graph"), ("C2", "random"), ("C4", "random"), ("C4", "graph")])
def test_device_chain_at_full_size(cfg_name, lmc_kind):
    torch = pytest.importorskip("torch")
    cfg = synth.CONFIGS[cfg_name]
    N = cfg.n_nodes
    pts, sph = synth.nodes(N, 3), synth.spheres(cfg.n_obstacles)
    Q = _scene_queries(cfg, sph)
    nq, r = len(Q), synth.ball_radius(N, 3)
    with Context(3, node_capacity=N) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        lists = ctx.extend_candidates(Q, r, RR)
        k = len(lists["idx"])
        if lmc_kind == "graph":
            _mirror_random_tree(ctx, N, seed=5)
            d_lmc = torch.empty(N, dtype=torch.float64, device="cuda:0")
            ctx._check(ctx._lib.rrtx_graph_cost_to_root_dev(ctx.handle, 0, d_lmc.data_ptr(), None))
            ctx.sync()
            lmc = d_lmc.cpu().numpy()
            assert lmc[0] == 0.0 and np.isinf(lmc).any() and np.isfinite(lmc).sum() > 0.9 * N
        else:
            lmc = _random_lmc(N, seed=6)
            safe = np.flatnonzero((np.diff(lists["offsets"]) > 0) & (lists["sample_unsafe"] == 0))[0]
            lmc[lists["idx"][lists["offsets"][safe]:lists["offsets"][safe + 1]]] = math.inf     # a sample among orphans only
            d_lmc = torch.from_numpy(lmc).to("cuda:0")
        ref = _reference(lists, lmc)
        # the inputs: all four statuses, many rewire lists, segments of one entry and segments longer than a wave's group
        seen = set(ref["status"].tolist())
        assert {SEL_OK, SEL_EMPTY, SEL_UNSAFE} <= seen and (lmc_kind == "graph" or SEL_NO_PARENT in seen)
        assert _ok_share_with_rewire(ref) >= 0.25 and len(ref["rw_node"]) > nq
        seg = np.diff(lists["offsets"])
        assert seg.max() > 32
        d = _Dev(torch, nq, k + 7, k)
        _extend_dev(ctx, d, Q, r)
        assert int(d.need.item()) == k
        got = d.select(ctx, d_lmc.data_ptr())
        assert got["rw_needed"] == len(ref["rw_node"])
        _assert_same(got, ref, (cfg_name, lmc_kind))
        longest = int(np.argmax(seg))                                  # the longest segment of the scene, by name
        lo, hi = ref["rw_offsets"][longest], ref["rw_offsets"][longest + 1]
        assert got["parent_idx"][longest] == ref["parent_idx"][longest]
        assert np.array_equal(got["rw_node"][lo:hi], ref["rw_node"][lo:hi])
        # the same through the context's own cost array, uploaded in two parts (a NaN and Inf travel as they are)
        ctx.node_cost_set(0, lmc[:N // 3])
        ctx.node_cost_set(N // 3, lmc[N // 3:])
        _assert_same(d.select(ctx, None), ref, "node_cost_set")
        # without the unsafe flags the unsafe samples are selected like the others
        ref_nu = _reference(lists, lmc, unsafe=False)
        assert SEL_UNSAFE not in ref_nu["status"]
        _assert_same(d.select(ctx, d_lmc.data_ptr(), unsafe=False), ref_nu, "no unsafe flags")
        # two-call pattern of the device form: the count is exact, nothing is written at or beyond rw_cap
        d.rwn.fill_(-7)
        small = d.select(ctx, d_lmc.data_ptr(), rw_cap=100)
        assert small["rw_needed"] == len(ref["rw_node"]) and np.array_equal(small["rw_offsets"], ref["rw_offsets"])
        rwn = d.rwn.cpu().numpy()
        assert np.array_equal(rwn[:100], ref["rw_node"][:100]) and (rwn[100:] == -7).all()


def test_device_form_edge_cases():
    torch = pytest.importorskip("torch")
    cfg = synth.CONFIGS["C2"]
    N = cfg.n_nodes
    pts, sph = synth.nodes(N, 3), synth.spheres(cfg.n_obstacles)
    Q = _scene_queries(cfg, sph)
    nq, r = len(Q), synth.ball_radius(N, 3)
    lmc = _random_lmc(N, seed=8)
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        lists = ctx.extend_candidates(Q, r, RR)
        k = len(lists["idx"])
        d_lmc = torch.from_numpy(lmc).to("cuda:0")
        d = _Dev(torch, nq, k, k)
        _extend_dev(ctx, d, Q, r)
        # every out-edge blocked: nobody gets a parent, no rewire entry
        blocked = dict(lists, hit_out=np.full(k, 2, dtype=np.uint8))
        ref = _reference(blocked, lmc)
        assert set(ref["status"].tolist()) == {SEL_NO_PARENT, SEL_EMPTY, SEL_UNSAFE} and len(ref["rw_node"]) == 0
        got = d.select(ctx, d_lmc.data_ptr(), hit_out=torch.full((k,), 2, dtype=torch.uint8, device="cuda:0"))
        _assert_same(got, ref, "all blocked")
        # the extend call overflowed its capacity: every status says so and nothing else is written
        d2 = _Dev(torch, nq, k // 2, k)
        _extend_dev(ctx, d2, Q, r)
        assert int(d2.need.item()) == k
        got = d2.select(ctx, d_lmc.data_ptr())
        assert (got["status"] == SEL_OVERFLOW).all()
        assert (got["parent_idx"] == -7).all() and (got["lmc_new"] == -7.0).all() and (got["rw_offsets"] == -7).all()
        assert got["rw_needed"] == -7 and (d2.rwn.cpu().numpy() == -7).all()
        # nq = 0: an empty CSR
        d0 = _Dev(torch, 0, 4, 4)
        d0.off.fill_(0)
        d0.need.fill_(0)
        got = d0.select(ctx, d_lmc.data_ptr())
        assert got["rw_needed"] == 0 and got["rw_offsets"][0] == 0 and (d0.st.cpu().numpy() == 77).all()
        # argument errors fail like the neighbours'
        with pytest.raises(RrtxError) as e:
            ctx.extend_select_dev(4, None, d.idx.data_ptr(), d.cost.data_ptr(), d.cost.data_ptr(), d.ho.data_ptr(),
                                  d.hi.data_ptr(), None, k, None, None, d.pi.data_ptr(), d.pe.data_ptr(), d.ln.data_ptr(),
                                  d.st.data_ptr(), d.rwo.data_ptr(), d.rwn.data_ptr(), d.rwv.data_ptr(), k, d.rwneed.data_ptr())
        assert e.value.code == _capi.RRTX_E_INVALID
        with pytest.raises(RrtxError) as e:
            ctx.node_cost_set(N - 1, [1.0, 2.0])
        assert e.value.code == _capi.RRTX_E_INVALID
    # all samples unsafe, and a tree of one node (every segment has one entry: the root, taken with <=)
    with Context(3) as ctx:
        ctx.nodes_append(np.zeros((1, 3)))
        ctx.spheres_set(np.array([[30.0, 30.0, 30.0, 3.0]]))
        Qu = np.array([30.0, 30.0, 30.0]) + np.random.default_rng(2).uniform(-1, 1, (70, 3))
        out = ctx.extend_select(Qu, 80.0, RR, lmc=[0.0])
        assert (out["status"] == SEL_UNSAFE).all() and (out["parent_idx"] == -1).all() and np.isinf(out["lmc_new"]).all()
        assert (out["rw_offsets"] == 0).all() and len(out["rw_node"]) == 0
        Q1 = np.random.default_rng(3).uniform(-9, 9, (70, 3))
        lists = ctx.extend_candidates(Q1, 20.0, RR)
        assert (np.diff(lists["offsets"]) == 1).all()
        out = ctx.extend_select(Q1, 20.0, RR, lmc=[0.0])
        _assert_same(out, _reference(lists, np.zeros(1)), "one entry")
        assert (out["status"] == SEL_OK).all() and np.array_equal(out["lmc_new"], lists["cost"])
        e = ctx.extend_select(np.zeros((0, 3)), 20.0, RR, lmc=[0.0])
        assert len(e["status"]) == 0 and e["rw_offsets"].tolist() == [0] and len(e["rw_node"]) == 0


# ---- synthetic device lists: the shared scan and the list walk at their edges ------------------------------------------
SYN_LENGTHS = np.array([0, 1, 7, 8, 9, 63, 64, 65, 300])
# the share of each length; the mean list length (7.0, 14.4, 27.5, 57.4) decides the lanes per sample: 8, 16, 32, 64
SYN_WEIGHTS = {8: [.25, .25, .2, .15, .12, .01, .01, .005, .005], 16: [.1, .1, .25, .25, .2, .03, .03, .03, .01],
               32: [.1, .1, .2, .2, .15, .08, .07, .07, .03], 64: [1 / 9] * 9}
SYN_NODES = 64


def _synthetic_lists(rng, nq, group):
    cnt = rng.choice(SYN_LENGTHS, nq, p=SYN_WEIGHTS[group])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = int(off[-1])
    idx = rng.integers(0, SYN_NODES, n).astype(np.int32)
    cost = rng.integers(0, 12, n) / 4.0                            # quarter integers: exact ties in lmc + cost
    ho = (rng.random(n) < 0.2).astype(np.uint8) * rng.choice(np.array([1, 2, 3], dtype=np.uint8), n)
    hi = (rng.random(n) < 0.2).astype(np.uint8) * rng.choice(np.array([1, 2, 3], dtype=np.uint8), n)
    uns = (rng.random(nq) < 0.05).astype(np.uint8)
    lmc = rng.integers(0, 40, SYN_NODES) / 4.0
    lmc[rng.random(SYN_NODES) < 0.15] = math.inf
    lmc[[5, 41]] = math.nan
    lmc[0] = 0.0
    return dict(offsets=off, idx=idx, cost=cost, hit_out=ho, hit_in=hi, sample_unsafe=uns), lmc


@pytest.mark.parametrize("nq", [0, 1, 3, 4, 5, 4095, 4096, 4097, 8193])
def test_synthetic_lists_across_scan_rounds(nq):
    """rrtx_extend_select_dev on lists written by the test over a tree of 64 nodes: sample counts around the scan's four
    counters per thread and its 4096-counter rounds, list lengths around every group size (empty and over-long lists in
    every group), exact ties, +Inf and NaN costs.  All eight outputs against select_numpy, exactly; then with rw_cap
    below rw_needed (the prefix is written, nothing beyond it, rw_needed is the full count) and with rw_offsets at an
    address that is only 8-byte aligned (the scan's one-by-one stores)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1000 + nq)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    groups = set()
    with Context(3) as ctx:
        ctx.nodes_append(np.random.default_rng(1).uniform(-5, 5, (SYN_NODES, 3)))
        for group in (8, 16, 32, 64):
            lists, lmc = _synthetic_lists(rng, nq, group)
            n = int(lists["offsets"][-1])
            ref = _reference(lists, lmc)
            mean = n // max(nq, 1)
            groups.add(min(g for g in (8, 16, 32, 64) if g >= mean or g == 64))
            if nq >= 4095:
                assert {SEL_OK, SEL_EMPTY, SEL_UNSAFE, SEL_NO_PARENT} == set(ref["status"].tolist())
                assert tie_samples(lists["offsets"], lists["idx"], lists["cost"], lists["hit_out"], lmc) >= 64
                assert len(ref["rw_node"]) > nq // 4
            d = _Dev(torch, nq, n + 3, max(len(ref["rw_node"]), 1))
            d.off[:nq + 1] = up(lists["offsets"])
            if n:
                d.idx[:n], d.cost[:n] = up(lists["idx"]), up(lists["cost"])
                d.ho[:n], d.hi[:n] = up(lists["hit_out"]), up(lists["hit_in"])
            if nq:
                d.un[:nq] = up(lists["sample_unsafe"])
            d.need.fill_(n)
            d_lmc = up(lmc)
            got = d.select(ctx, d_lmc.data_ptr())
            assert got["rw_needed"] == len(ref["rw_node"]), (nq, group)
            got["rw_offsets"] = got["rw_offsets"][:nq + 1]
            _assert_same(got, ref, (nq, group))
            # rw_cap below rw_needed
            need = len(ref["rw_node"])
            if need >= 2:
                small_cap = need // 2
                d.rwn.fill_(-7); d.rwv.fill_(-7.0); d.rwo.fill_(-7); d.rwneed.fill_(-7)
                small = d.select(ctx, d_lmc.data_ptr(), rw_cap=small_cap)
                assert small["rw_needed"] == need and np.array_equal(small["rw_offsets"][:nq + 1], ref["rw_offsets"])
                rwn, rwv = d.rwn.cpu().numpy(), d.rwv.cpu().numpy()
                assert np.array_equal(rwn[:small_cap], ref["rw_node"][:small_cap]) and (rwn[small_cap:] == -7).all()
                assert np.array_equal(rwv[:small_cap], ref["rw_value"][:small_cap]) and (rwv[small_cap:] == -7.0).all()
            # rw_offsets one int64 past an aligned address
            odd = torch.full((nq + 2,), -7, dtype=torch.int64, device="cuda:0")
            ctx.extend_select_dev(nq, d.off.data_ptr(), d.idx.data_ptr(), d.cost.data_ptr(), d.cost.data_ptr(), d.ho.data_ptr(),
                                  d.hi.data_ptr(), d.need.data_ptr(), d.cap, d.un.data_ptr(), d_lmc.data_ptr(), d.pi.data_ptr(),
                                  d.pe.data_ptr(), d.ln.data_ptr(), d.st.data_ptr(), odd.data_ptr() + 8, d.rwn.data_ptr(),
                                  d.rwv.data_ptr(), d.rw_cap, d.rwneed.data_ptr())
            ctx.sync()
            odd = odd.cpu().numpy()
            assert odd[0] == -7 and np.array_equal(odd[1:], ref["rw_offsets"]), (nq, group, "unaligned rw_offsets")
    if nq >= 4095:
        assert groups == {8, 16, 32, 64}, groups


# ---- the fused host-pointer call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("obstacles", ["spheres", "polygons"])
@pytest.mark.parametrize("registered", [False, True])
def test_fused_call_equals_the_chain(obstacles, registered):
    torch = pytest.importorskip("torch")
    cfg = synth.CONFIGS["C2"]
    N = cfg.n_nodes
    pts, sph = synth.nodes(N, 3), synth.spheres(cfg.n_obstacles)
    Q = _scene_queries(cfg, sph)
    nq, r = len(Q), synth.ball_radius(N, 3)
    lmc = _random_lmc(N, seed=9)
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        if obstacles == "spheres":
            ctx.spheres_set(sph)
        else:
            ctx.polygons_set(synth.polygons(48))
            ctx.set_option(_capi.RRTX_OPT_EXTEND_OBSTACLES, 1)
        lists = ctx.extend_candidates(Q, r, RR)
        k = len(lists["idx"])
        ref = _reference(lists, lmc)
        assert (lists["hit_out"] != 0).any() and lists["sample_unsafe"].any()
        assert _ok_share_with_rewire(ref) >= 0.25
        d = _Dev(torch, nq, k, k)
        _extend_dev(ctx, d, Q, r)
        chain = d.select(ctx, torch.from_numpy(lmc).to("cuda:0").data_ptr())
        _assert_same(chain, ref, "chain")
        # a first call whose neighbour count exceeds the internal capacity still answers (and has grown it)
        ctx.set_option(_capi.RRTX_OPT_SELECT_LIST_CAP, 64)
        nrw = len(ref["rw_node"])
        bufs = ctx.select_out_buffers(nq, nrw + 64, register=registered)      # (room for the changed cost below)
        out = ctx.extend_select(Q, r, RR, lmc=lmc, out=bufs)
        assert ctx.get_option(_capi.RRTX_OPT_SELECT_LIST_CAP) >= k and out["n_neighbors"] == k
        for name, got in (("fused", out), ("fused again", ctx.extend_select(Q, r, RR, lmc=lmc, out=bufs))):
            _assert_same(got, chain, name)
            for key in ("nearest_idx", "nearest_dist", "sample_unsafe"):
                assert np.array_equal(got[key], lists[key]), (name, key)
        # the context's own cost array in the place of the caller's
        ctx.node_cost_set(0, lmc)
        _assert_same(ctx.extend_select(Q, r, RR, out=bufs), ref, "node_cost_set")
        ctx.node_cost_set(7, [0.25])
        lmc2 = lmc.copy(); lmc2[7] = 0.25
        _assert_same(ctx.extend_select(Q, r, RR, out=bufs), _reference(lists, lmc2), "one value changed")
        # a too-small rw_cap: RRTX_E_CAPACITY with the right count, per-sample outputs already valid; then it fits
        pi, pe, ln, st = (np.empty(nq, dtype=t) for t in (np.int32, np.int64, np.float64, np.uint8))
        rwo = np.empty(nq + 1, dtype=np.int64)
        rwn, rwv = np.full(nrw, -7, dtype=np.int32), np.empty(nrw, dtype=np.float64)
        need, lneed = C.c_int64(), C.c_int64()
        call = lambda cap: ctx._lib.rrtx_extend_select(
            ctx.handle, Q.ctypes.data, nq, r, RR, lmc.ctypes.data, pi.ctypes.data, pe.ctypes.data, ln.ctypes.data,
            st.ctypes.data, rwo.ctypes.data, rwn.ctypes.data, rwv.ctypes.data, cap, C.byref(need), None, None, None, None,
            None, None, None, None, 0, C.byref(lneed))
        assert call(nrw - 1) == _capi.RRTX_E_CAPACITY and need.value == nrw and (rwn == -7).all()
        assert np.array_equal(st, ref["status"]) and np.array_equal(rwo, ref["rw_offsets"])
        assert call(int(need.value)) == _capi.RRTX_OK and lneed.value == k
        _assert_same(dict(status=st, parent_idx=pi, parent_entry=pe, lmc_new=ln, rw_offsets=rwo, rw_node=rwn, rw_value=rwv),
                     ref, "second call")
        # the growing wrapper, and the lists themselves on request
        full = ctx.extend_select(Q, r, RR, lmc=lmc, rw_cap=16, want_lists=True, cap=16)
        _assert_same(full, ref, "wrapper")
        for key in ("offsets", "idx", "cost", "hit_out", "hit_in"):
            assert np.array_equal(full[key], lists[key]), key
        with pytest.raises(RrtxError) as e:
            ctx.extend_select(Q, r, RR, lmc=lmc, out=ctx.select_out_buffers(nq, nrw, list_cap=k - 1))
        assert e.value.code == _capi.RRTX_E_CAPACITY
    with Context(4) as ctx4:
        ctx4.nodes_append(synth.nodes(64, 4))
        with pytest.raises(RrtxError) as e:
            ctx4.extend_select(synth.queries(4, 4), 5.0, RR, lmc=np.zeros(64))
        assert e.value.code == _capi.RRTX_E_STATE


def test_registered_buffers_are_released_with_the_context():
    ctx = Context(3)
    ctx.nodes_append(synth.nodes(2000, 3))
    ctx.spheres_set(synth.spheres(8))
    bufs = ctx.select_out_buffers(700, 40_000, register=True)
    assert len(ctx._registered) == len(bufs)
    out = ctx.extend_select(synth.queries(700, 3), 12.0, RR, lmc=np.zeros(2000), out=bufs)
    assert (out["status"] != SEL_OVERFLOW).all()
    del bufs, out                      # the caller drops its references: the context still holds the arrays
    assert all(a.flags["C_CONTIGUOUS"] for a in ctx._registered)
    ctx.close()
    assert ctx._registered == []


# ---- exact ties ----------------------------------------------------------------------------------------------------
def _lattice_scene():
    rng = np.random.default_rng(3)
    P = np.unique(rng.integers(0, 64, (20000, 3)) / 4.0, axis=0)
    P = P[rng.permutation(len(P))]
    Q = rng.integers(0, 64, (2048, 3)) / 4.0
    lmc = rng.integers(0, 40, len(P)) / 4.0
    lmc[0] = 0.0
    sph = np.concatenate([rng.integers(8, 56, (6, 3)) / 4.0, np.full((6, 1), 1.5)], axis=1)
    return P, Q, lmc, sph


def test_lattice_scene_where_ties_decide():
    torch = pytest.importorskip("torch")
    P, Q, lmc, sph = _lattice_scene()
    nq = len(Q)
    with Context(3) as ctx:
        ctx.nodes_append(P)
        ctx.spheres_set(sph)
        lists = ctx.extend_candidates(Q, 1.0, RR)
        k = len(lists["idx"])
        ref = _reference(lists, lmc)
        assert tie_samples(lists["offsets"], lists["idx"], lists["cost"], lists["hit_out"], lmc) >= 16
        assert len(ref["rw_node"]) > 1000 and (lists["hit_out"] != 0).any()
        d = _Dev(torch, nq, k, k)
        _extend_dev(ctx, d, Q, 1.0)
        _assert_same(d.select(ctx, torch.from_numpy(lmc).to("cuda:0").data_ptr()), ref, "lattice chain")
        _assert_same(ctx.extend_select(Q, 1.0, RR, lmc=lmc), ref, "lattice fused")


# ---- Dubins lists: cost_out != cost_in, flag bytes of value 2 ----------------------------------------------------------
@pytest.mark.parametrize("has_time", [False, True])
def test_dubins_lists(has_time):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(23)
    if has_time:
        d_env = json.load(open(os.path.join(ROOT, "golden", "env_inputs.json")))
        polys = [np.array(p, dtype=np.float64) for p in d_env["rand_StaticTime_7_polygons"]][::-1]
        paths = [np.array(p, dtype=np.float64) for p in d_env["rand_StaticTime_7_paths"]][::-1]
        n, nq, r, r_min = 6000, 256, 9.0, 2.0
        pts, Q = synth.nodes(n, 4), synth.queries(nq, 4)
        pts[:, 2] = rng.uniform(10.0, 35.0, n)
        Q[:, 2] = rng.uniform(10.0, 35.0, nq)
    else:
        n, nq, r, r_min = 12_000, 300, 9.0, 1.0
        pts, Q, polys = synth.nodes(n, 4), synth.queries(nq, 4), synth.polygons(24)
    lmc = rng.uniform(0.0, 80.0, n)
    lmc[rng.random(n) < 0.1] = math.inf
    lmc[0] = 0.0
    with Context(4) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        if has_time:
            ctx.polygons_set(polys, kinds=[6] * len(polys), paths=paths)
            ctx.set_space_has_time(True)
            ctx.set_dubins_velocity(5.0, 30.0)
        else:
            ctx.polygons_set(polys)
        lists = ctx.extend_candidates_dubins(Q, r, RR, r_min)
        k = len(lists["idx"])
        assert k > 1000 and not np.array_equal(lists["cost_out"], lists["cost_in"])
        if has_time:
            assert (lists["hit_out"] == 2).any() and (lists["hit_in"] == 2).any()      # !validMove alone blocks an edge
        ref = _reference(lists, lmc, cost_in="cost_in")
        assert (ref["status"] == SEL_OK).sum() > nq // 4 and len(ref["rw_node"]) > 100
        d = _Dev(torch, nq, k + 3, k, dubins=True)
        dq = torch.from_numpy(Q).to("cuda:0")
        ctx.extend_candidates_dubins_dev(dq.data_ptr(), nq, r, RR, r_min, d.off.data_ptr(), d.idx.data_ptr(), d.key.data_ptr(),
                                         d.cost.data_ptr(), d.cost_in.data_ptr(), None, None, d.ho.data_ptr(), d.hi.data_ptr(),
                                         d.cap, d.need.data_ptr(), d.ni.data_ptr(), d.nd.data_ptr(), d.un.data_ptr())
        ctx.sync()
        assert int(d.need.item()) == k
        _assert_same(d.select(ctx, torch.from_numpy(lmc).to("cuda:0").data_ptr()), ref, ("dubins", has_time))


# ---- the planner's loop ----------------------------------------------------------------------------------------------
def _grow_select(be, n_iter, seed):
    """_grow of tests/test_gpu_planner_loop.py with drrt.extend_select in the place of the point check, the range
    search, findBestParent's loop and the rewire loop; rrtLMC travels to the device one changed value at a time."""
    from test_gpu_planner_loop import BALL_CONSTANT, DELTA, HI, LO
    rng = np.random.default_rng(seed)
    pos = [np.array([15.0, 15.0, 15.0])]
    parent, lmc = [-1], [0.0]
    be.insert(pos[0])
    be.nodes[0].rrtLMC = 0.0
    be.tree.ctx.node_cost_set(0, [0.0])
    statuses = set()
    for _ in range(n_iter):
        p = rng.uniform(LO, HI, 3)
        n = len(pos)
        r = min(DELTA, BALL_CONSTANT * ((math.log(1 + n) / n) ** (1.0 / 3)))
        out = drrt.extend_select(be.tree, be.S, [p], r)
        # (a parent without a list position: the ball was empty and the closestNode rule linked the sample)
        statuses.add("empty" if out["status"][0] == SEL_OK and out["parent_entry"][0] < 0 else int(out["status"][0]))
        if out["status"][0] != SEL_OK:
            continue
        best, best_parent = float(out["lmc_new"][0]), int(out["parent_idx"][0])
        new = be.insert(p)
        assert new == n
        pos.append(p); parent.append(best_parent); lmc.append(best)
        be.nodes[new].rrtLMC = best
        be.tree.ctx.node_cost_set(new, [best])
        for j, v in zip(out["rw_node"], out["rw_value"]):
            parent[j] = new
            lmc[j] = float(v)
            be.nodes[j].rrtLMC = float(v)
            be.tree.ctx.node_cost_set(int(j), [float(v)])
    return (np.array(pos), np.array(parent), np.array(lmc)), statuses


@pytest.mark.parametrize("cull", [1, 2])
def test_planner_loop_grows_the_same_tree(oracle, cull):
    from test_gpu_planner_loop import _CpuBackend, _GpuBackend, _grow, _spheres
    sph = _spheres()
    n_iter = 2600 if cull == 2 else 1200
    g, statuses = _grow_select(_GpuBackend(sph, cull), n_iter, seed=7)
    c = _grow(_CpuBackend(oracle, sph), n_iter, seed=7)
    assert len(g[0]) == len(c[0]) and len(g[0]) > 0.7 * n_iter
    assert np.array_equal(g[0], c[0])
    assert np.array_equal(g[1], c[1])
    assert np.array_equal(g[2], c[2])
    assert {"empty", SEL_OK, SEL_UNSAFE} <= statuses          # the closestNode rule of an empty ball ran
