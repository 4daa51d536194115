"""nn_finish_kernel behind `if (!small)`: the loop over long or overflowed lists -- placement by counting in index bins,
the crowd rule, the bitonic network at every padded size, rank counting over global memory, the gather from the shared
overflow list with its packed flags, the pre-scattered form, the growing bucket multiplier, the cut by the caller's
capacity and the nearest across eight waves -- each against the CPU oracle with == (keys as bit patterns).

The lists are those of finish_lists_model.py: exact lengths on both sides of 64, 128, ..., 2048, 8192, chosen index sets
on both sides of the crowd of 128, and a restatement of plan_radius that says which call of a context gathers, which is
pre-scattered and which finds everything in the buckets.  test_finish_list_scenes.py holds the scenes to that on the
oracle alone."""
import numpy as np
import pytest

import finish_lists_model as M
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

SCENES = ("huge", "big", "tight")
CULLS = (2, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_lists(got, ref, label):
    off, idx, dist = got
    assert np.array_equal(off, ref["offsets"]), f"{label}: offsets"
    assert np.array_equal(idx, ref["idx"]), f"{label}: idx"
    assert np.array_equal(bits(dist), bits(ref["key"])), f"{label}: dist"


def context(name, cull, mult=None):
    ctx = Context(3)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
    if mult is not None:
        ctx.set_option(_capi.RRTX_OPT_BUCKET_MULT, mult)
    ctx.nodes_append(M.scene(name)["pts"])
    return ctx


# ---- lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULLS)
@pytest.mark.parametrize("name", SCENES)
def test_five_calls_on_one_context(oracle, name, cull):
    """cap = the exact total; the multiplier the library holds after every call is the model's, so the call took the
    model's buckets: gathered in the kernel, pre-scattered, or all in the buckets"""
    s, ref = M.scene(name), M.reference(oracle, name)
    nq, total = len(s["want"]), len(ref["idx"])
    plan = M.calls(s["want"], nq, total, 5)
    if name == "huge":
        assert {c["state"] for c in plan} == {"gather", "prescattered", "in bucket"} and M.build(total, nq)
    with context(name, cull) as ctx:
        for k, c in enumerate(plan):
            got = ctx.nn_radius(s["Q"], s["r"], cap=total)
            assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == c["mult"], (name, cull, k)
            assert_lists(got, ref, f"{name}, cull {cull}, call {k + 1} ({c['state']}, buckets of {c['bcap']})")


@pytest.mark.parametrize("cull", CULLS)
@pytest.mark.parametrize("name", SCENES)
def test_widest_buckets_from_the_start(oracle, name, cull):
    s, ref = M.scene(name), M.reference(oracle, name)
    with context(name, cull, mult=16) as ctx:
        assert_lists(ctx.nn_radius(s["Q"], s["r"], cap=len(ref["idx"])), ref, f"{name}, cull {cull}, multiplier 16")
        assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == 16


# ---- the other build on the same lists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULLS)
def test_big_in_the_long_list_build(oracle, cull):
    """room for 513 entries a sample: the lists of big are placed by counting, none is sorted by the network"""
    s, ref = M.scene("big"), M.reference(oracle, "big")
    nq = len(s["want"])
    cap = 513 * nq
    assert M.build(cap, nq) and cap >= len(ref["idx"])
    plan = M.calls(s["want"], nq, cap, 3)
    with context("big", cull) as ctx:
        for k, c in enumerate(plan):
            got = ctx.nn_radius(s["Q"], s["r"], cap=cap)
            assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == c["mult"]
            assert_lists(got, ref, f"big, cap {cap}, cull {cull}, call {k + 1} ({c['state']})")


@pytest.mark.parametrize("cull", CULLS)
def test_huge_in_the_normal_build(oracle, cull):
    """the lists of huge up to 8192 entries among so many empty balls that cap = total selects the normal build: the
    placed and the crowded lists alike take the network up to 2048 entries and rank counting beyond"""
    s = M.scene("huge")
    keep, nq = M.normal_build_batch("huge")
    Q = M.padded("huge", keep, nq)
    ref = M._once(("normal build", "huge"), lambda: M.lists(oracle, "huge", Q))
    want = np.diff(ref["offsets"])
    total = len(ref["idx"])
    assert np.array_equal(want[:len(keep)], s["want"][keep]) and not want[len(keep):].any() and not M.build(total, nq)
    plan = M.calls(want, nq, total, 5)
    assert plan[0]["state"] == "gather" and plan[1]["state"] == "prescattered"
    with context("huge", cull) as ctx:
        for k, c in enumerate(plan):
            got = ctx.nn_radius(Q, s["r"], cap=total)
            assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == c["mult"]
            assert_lists(got, ref, f"huge in the normal build, cull {cull}, call {k + 1} ({c['state']})")


# ---- flags and nearest -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULLS)
@pytest.mark.parametrize("name", SCENES)
def test_flags_and_nearest(oracle, name, cull):
    s, ext = M.scene(name), M.reference_extend(oracle, name)
    nq, total = len(s["want"]), len(ext["idx"])
    plan = M.calls(s["want"], nq, total, 3)
    empty = s["want"] == 0
    with context(name, cull) as ctx:
        ctx.spheres_set(s["sph"])
        for k, c in enumerate(plan):
            label = f"{name}, cull {cull}, call {k + 1} ({c['state']})"
            out = ctx.extend_candidates(s["Q"], s["r"], M.RR, cap=total)
            assert ctx.get_option(_capi.RRTX_OPT_BUCKET_MULT) == c["mult"], label
            assert_lists((out["offsets"], out["idx"], out["cost"]), ext, label)
            for f in ("hit_out", "hit_in"):
                bad = np.flatnonzero(out[f] != ext[f])
                owner = np.searchsorted(ext["offsets"], bad[:1], side="right") - 1
                assert len(bad) == 0, f"{label}: {len(bad)} {f} flags differ, the first in the list of sample {owner}"
            ni, nd = out["nearest_idx"], out["nearest_dist"]
            bad = np.flatnonzero(~empty & ((ni != ext["low_idx"]) | (bits(nd) != bits(ext["low_key"]))))
            assert len(bad) == 0, f"{label}: nearest of the lists of samples {bad[:8]} (lengths {s['want'][bad[:8]]})"
            assert np.array_equal(ni[empty], ext["nearest_idx"][empty]), f"{label}: nearest of empty balls"
            assert np.array_equal(bits(nd[empty]), bits(ext["nearest_dist"][empty])), f"{label}: nearest of empty balls"
            assert not out["sample_unsafe"].any()


# ---- capacity --------------------------------------------------------------------------------------------------------------
def caps_of(name):
    """capacities that end inside a list: (label, cap)"""
    s = M.scene(name)
    off = np.r_[0, np.cumsum(s["want"])]
    total = int(off[-1])

    def inside(kind, L):
        j, = [j for j in range(len(s["want"])) if s["kind"][j] == kind and s["want"][j] == L]
        return int(off[j]) + L // 2 + 1
    if name == "huge":
        caps = [("inside the list of 8193", inside("spread", 8193)), ("inside a crowded list", inside("block", 8192))]
        assert all(M.build(c, len(s["want"])) for _, c in caps)          # the long-list build cuts them
    else:
        caps = [("inside the list of 2560", inside("spread", 2560))]
    return caps + [("40", 40), ("the total", total)]


@pytest.mark.parametrize("warm", (True, False))
@pytest.mark.parametrize("name", ("huge", "big"))
def test_capacity_smaller_than_the_need(oracle, name, warm):
    """offsets and the count stay exact and nothing at or behind cap is written; warm: every capacity after a call on
    the same context that overflowed (wider buckets, possibly pre-scattered), otherwise on a fresh context, where the
    kernel gathers the overflow records itself and its guard dst < out_cap is what keeps them in front of cap"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    s, ref = M.scene(name), M.reference(oracle, name)
    nq, need = len(s["want"]), len(ref["idx"])
    assert M.calls(s["want"], nq, need, 1)[0]["overflow"] > 0
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        d_q = torch.from_numpy(s["Q"]).to(dev)

        def call(ctx, cap):
            d_off = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
            d_idx = torch.full((need + 64,), -7, dtype=torch.int32, device=dev)
            d_dist = torch.full((need + 64,), -7.0, dtype=torch.float64, device=dev)
            d_need = torch.zeros(1, dtype=torch.int64, device=dev)
            st.synchronize()
            ctx.nn_radius_dev(d_q.data_ptr(), s["r"], nq, d_off.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), cap,
                              d_need.data_ptr())
            st.synchronize()
            return int(d_need.item()), d_off.cpu().numpy(), d_idx.cpu().numpy(), d_dist.cpu().numpy()

        def check(ctx, label, cap):
            got_need, off, idx, dist = call(ctx, cap)
            assert got_need == need and np.array_equal(off, ref["offsets"]), (label, cap)
            if cap == need:
                assert np.array_equal(idx[:cap], ref["idx"]) and np.array_equal(bits(dist[:cap]), bits(ref["key"])), label
            assert (idx[cap:] == -7).all() and (dist[cap:] == -7.0).all(), (label, cap)

        if warm:
            with context(name, 2) as ctx:
                ctx.set_stream(st.cuda_stream)
                check(ctx, "the overflowing call", need)
                for label, cap in caps_of(name):
                    check(ctx, label, cap)
                ctx.set_stream(None)
        else:
            for label, cap in caps_of(name):
                with context(name, 2) as ctx:
                    ctx.set_stream(st.cuda_stream)
                    check(ctx, label, cap)
                    ctx.set_stream(None)
