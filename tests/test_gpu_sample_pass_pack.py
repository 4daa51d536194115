"""The sample pass of the fused extend() route runs in the pack launch (pack_sample_role): it decides sample_unsafe
and leaves every sample's sphere list in a per-query record that the tile kernel reads by owner.  Every case here is
held three ways, bit for bit over all eight extend fields: against the CPU oracle, between RRTX_OPT_TUNE 0 and 4 (the
tile kernel places the copies itself / the place pass does), and against RRTX_OPT_NN_CULL = 0, the two-kernel route
with sample_spheres_kernel.  Each test first asserts ON THE REFERENCE that the case it is there for occurs.

One tree for all cases: 9 001 uniform nodes in the +-50 box, r = ball_radius(9001, 3) = 8, robot radius 0.5."""
import numpy as np
import pytest

from rrtqx_3d_amd import _capi, synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

N = 9001
ROBOT_RADIUS = 0.5
GROUP = 16             # consecutive samples per wave pair of the sample role, = samples per tile
LIST_CAP = 8           # kSphListCap
QUEUE = 128            # near pairs a group queues (two waves x 64) before it evaluates them on the spot
EXTEND_FIELDS = ("offsets", "idx", "cost", "hit_out", "hit_in", "nearest_idx", "nearest_dist", "sample_unsafe")
NO_SPHERES = np.zeros((0, 4))
_CACHE = {}


def _tree():
    if "pts" not in _CACHE:
        _CACHE["pts"] = synth.nodes(N, 3)
        _CACHE["r"] = synth.ball_radius(N, 3)
    return _CACHE["pts"], _CACHE["r"]


def _reference(oracle, Q, r, sph):
    """the oracle's extend() preamble for the samples Q on the module's tree (the trees are built once)"""
    pts, _ = _tree()
    if "trees" not in _CACHE:
        _CACHE["trees"] = oracle.TreeSet(3, pts)
    return oracle.extend_candidates_batch(_CACHE["trees"], Q, r, pts, oracle.make_spheres(sph), ROBOT_RADIUS)


def _ctx(sph):
    pts, _ = _tree()
    ctx = Context(3, node_capacity=N)
    ctx.nodes_append(pts)
    if sph is not None:
        ctx.spheres_set(sph)
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    return ctx


def _three_ways(oracle, ctx, Q, r, ref, label):
    """the fused route (both placements) and the two-kernel route against each other and against the reference;
    returns the fused route's result"""
    outs = []
    for cull, tune, route in ((2, 0, 2), (2, 4, 1), (0, 0, 0)):     # RRTX_OPT_LAST_PLACEMENT: 2 tile kernel, 1 place pass
        ctx.set_option(_capi.RRTX_OPT_NN_CULL, cull)
        ctx.set_option(_capi.RRTX_OPT_TUNE, tune)
        outs.append(ctx.extend_candidates(Q, r, ROBOT_RADIUS))
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == route
    ctx.set_option(_capi.RRTX_OPT_NN_CULL, 2)
    ctx.set_option(_capi.RRTX_OPT_TUNE, 0)
    new, old, two = outs
    oracle.assert_same_results(old, new, EXTEND_FIELDS, label=f"{label}: RRTX_OPT_TUNE 4 against 0: ")
    oracle.assert_same_results(two, new, EXTEND_FIELDS, label=f"{label}: RRTX_OPT_NN_CULL 0 against 2: ")
    # a sample with a NaN coordinate orders against no node: the device answers nearest (INT_MAX, inf) where the
    # reference's kdFindNearest keeps its seed (root, NaN) -- those two fields are compared on the other samples
    nan = np.isnan(np.asarray(Q)).any(axis=1)
    if nan.any():
        assert (new["nearest_idx"][nan] == 0x7fffffff).all() and np.isinf(new["nearest_dist"][nan]).all()
        oracle.assert_same_results(new, ref, tuple(f for f in EXTEND_FIELDS if not f.startswith("nearest")),
                                   label=f"{label}: ")
        keep = np.flatnonzero(~nan)
        oracle.assert_same_results(oracle.take_samples(new, keep), oracle.take_samples(ref, keep), EXTEND_FIELDS,
                                   names=keep, label=f"{label}: ")
    else:
        oracle.assert_same_results(new, ref, EXTEND_FIELDS, label=f"{label}: ")
    return new


def _both_values(a):
    a = np.asarray(a)
    return bool((a == 0).any() and (a != 0).any())


# ---------------------------------------------------------------------------------------------- the cases' inputs
def spheres(M, seed=None):
    """synth.spheres with sphere 0 moved onto a node of the tree: the edges that end at that node collide"""
    sph = synth.spheres(M) if seed is None else synth.spheres(M, seed=seed)
    sph[0, :3] = _tree()[0][17] + np.array([0.3, 0.0, 0.0])
    return sph


def batch_queries(B, sph):
    """B samples; sample 0 sits 0.05 outside the inflated surface of sphere 0 (safe; of its edges the one to the
    node inside that sphere collides) and sample 1 at the centre of sphere 1 (unsafe), so that even the smallest
    batches meet both answers"""
    Q = synth.queries(B, 3, seed=100 + B)
    Q[0] = sph[0, :3] + np.array([sph[0, 3] + ROBOT_RADIUS + 0.05, 0.0, 0.0])
    if B > 1:
        Q[1] = sph[1, :3]
    return Q


def overflow_case():
    """40 spheres of radius 1 - 2 within 1.0 of P; samples 32 .. 47 (one aligned group) within 0.5 of P"""
    rng = np.random.default_rng(7)
    P = np.array([11.0, -7.0, 23.0])

    def within(n, d):
        v = rng.normal(size=(n, 3))
        return P + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.0, d, (n, 1))
    sph = np.concatenate([within(40, 1.0), rng.uniform(1.0, 2.0, (40, 1))], axis=1)
    Q = synth.queries(64, 3, seed=77)
    Q[32:48] = within(16, 0.5)
    return Q, sph


def non_finite_case():
    """NaN, +-inf and 1e300 in each coordinate, mixed into the aligned group 16 .. 31 with ordinary samples"""
    Q = synth.queries(48, 3, seed=31)
    k = 16
    for c in range(3):
        for v in (np.nan, np.inf, -np.inf, 1e300):
            Q[k, c] = v
            k += 1
    assert k == 28                    # samples 28 .. 31 of the group stay ordinary
    return Q


def no_neighbour_case(sph):
    """a radius so small that no ball holds a node; every fourth sample at a sphere's centre"""
    Q = synth.queries(40, 3, seed=55)
    Q[::4] = sph[:10, :3]
    return Q, 1e-4


# --------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 1000])
def test_batch_sizes(oracle, B):
    """partial groups, a partial last workgroup of either role, several parts per tile.  Both hit flags take both
    values at every size; sample_unsafe does at every size that has two samples (one sample has one answer: B = 1
    meets the safe one here and B >= 2 meet both)"""
    _, r = _tree()
    sph = spheres(64)
    Q = batch_queries(B, sph)
    ref = _reference(oracle, Q, r, sph)
    assert _both_values(ref["hit_out"]) and _both_values(ref["hit_in"])
    assert ref["sample_unsafe"][0] == 0
    if B > 1:
        assert _both_values(ref["sample_unsafe"])
    with _ctx(sph) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, f"B = {B}")


@pytest.mark.parametrize("M", [1, 2, 3, 255, 256])
def test_sphere_counts(oracle, M):
    """odd pair tail of the reach table, one and two passes of a group over it"""
    _, r = _tree()
    sph = spheres(M)
    Q = batch_queries(40, sph if M > 1 else np.concatenate([sph, sph]))
    ref = _reference(oracle, Q, r, sph)
    assert _both_values(ref["hit_out"]) and _both_values(ref["sample_unsafe"])
    with _ctx(sph) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, f"{M} spheres")


def test_no_spheres_at_all(oracle):
    _, r = _tree()
    Q = synth.queries(40, 3, seed=5)
    ref = _reference(oracle, Q, r, NO_SPHERES)
    assert len(ref["idx"]) > 5 * len(Q) and not ref["hit_out"].any() and not ref["sample_unsafe"].any()
    with _ctx(None) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, "no spheres")


def test_sphere_list_replaced_between_calls(oracle):
    """A, then B, then empty on one context: nothing stale is read from the per-sample records"""
    _, r = _tree()
    A, Bs = spheres(64), synth.spheres(48, seed=991)
    Q = batch_queries(100, A)
    Q[2] = Bs[0, :3]                  # unsafe under B only
    refs = [_reference(oracle, Q, r, s) for s in (A, Bs, NO_SPHERES)]
    assert refs[0]["sample_unsafe"][1] == 1 and refs[1]["sample_unsafe"][1] == 0
    assert refs[0]["sample_unsafe"][2] == 0 and refs[1]["sample_unsafe"][2] == 1
    assert refs[0]["hit_out"].any() and refs[1]["hit_out"].any()
    assert not np.array_equal(refs[0]["hit_out"], refs[1]["hit_out"])
    assert not refs[2]["hit_out"].any() and not refs[2]["sample_unsafe"].any()
    with _ctx(A) as ctx:
        _three_ways(oracle, ctx, Q, r, refs[0], "list A")
        ctx.spheres_set(Bs)
        _three_ways(oracle, ctx, Q, r, refs[1], "list B")
        ctx.spheres_set(NO_SPHERES)
        _three_ways(oracle, ctx, Q, r, refs[2], "empty list")


def test_list_overflow_and_queue_overflow_together(oracle):
    _, r = _tree()
    Q, sph = overflow_case()
    # from the inputs: every sample of the group has more than LIST_CAP spheres with |centre - sample| <= r + 0.5 +
    # radius, and the group has more such pairs than its two queues hold
    d = np.linalg.norm(Q[32:48, None, :] - sph[None, :, :3], axis=2)
    near = d <= r + ROBOT_RADIUS + sph[None, :, 3]
    assert (near.sum(axis=1) > LIST_CAP).all() and near.sum() > QUEUE
    assert 32 % GROUP == 0
    ref = _reference(oracle, Q, r, sph)
    assert ref["sample_unsafe"][32:48].all() and _both_values(ref["sample_unsafe"]) and _both_values(ref["hit_out"])
    with _ctx(sph) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, "list and queue overflow")


def test_non_finite_and_huge_samples(oracle):
    """the probe of such a sample is +inf: every (sample, sphere) pair goes to the exact part"""
    _, r = _tree()
    sph = spheres(64)
    Q = non_finite_case()
    assert 16 % GROUP == 0 and np.isfinite(Q[28:32]).all() and (np.abs(Q[28:32]) <= 50.0).all()
    bad = ~np.isfinite(Q).all(axis=1) | (np.abs(Q) >= 1e300).any(axis=1)
    assert bad.sum() == 12 and bad[16:28].all()
    ref = _reference(oracle, Q, r, sph)
    assert (np.diff(ref["offsets"])[16:28] == 0).all() and (np.diff(ref["offsets"])[28:32] > 0).all()
    with _ctx(sph) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, "non-finite and huge samples")


def test_no_neighbours_possible(oracle):
    """sample_unsafe is decided although no tile has anything to list or screen"""
    sph = spheres(64)
    Q, r = no_neighbour_case(sph)
    ref = _reference(oracle, Q, r, sph)
    assert ref["offsets"][-1] == 0 and _both_values(ref["sample_unsafe"])
    with _ctx(sph) as ctx:
        _three_ways(oracle, ctx, Q, r, ref, "no neighbours possible")


def test_workspace_sizing(oracle):
    """B = 1000 and then B = 17 on one context"""
    _, r = _tree()
    sph = spheres(64)
    with _ctx(sph) as ctx:
        for B in (1000, 17):
            Q = batch_queries(B, sph)
            ref = _reference(oracle, Q, r, sph)
            assert _both_values(ref["sample_unsafe"]) and _both_values(ref["hit_out"])
            _three_ways(oracle, ctx, Q, r, ref, f"B = {B} after the larger batch" if B == 17 else f"B = {B}")


def test_null_sample_unsafe(oracle):
    """extend_candidates_dev takes a null sample_unsafe: the other fields are what they are with it"""
    import torch
    _, r = _tree()
    sph = spheres(64)
    B = 100
    Q = batch_queries(B, sph)
    ref = _reference(oracle, Q, r, sph)
    assert _both_values(ref["sample_unsafe"]) and _both_values(ref["hit_out"])
    dev = torch.device("cuda", 0)
    with _ctx(sph) as ctx:
        cap = len(ref["idx"]) + 5
        d_q = torch.from_numpy(Q).to(dev)
        d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        d_idx = torch.empty(cap, dtype=torch.int32, device=dev)
        d_cost = torch.empty(cap, dtype=torch.float64, device=dev)
        d_ho = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_hi = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_need = torch.zeros(1, dtype=torch.int64, device=dev)
        d_ni = torch.empty(B, dtype=torch.int32, device=dev)
        d_nd = torch.empty(B, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.extend_candidates_dev(d_q.data_ptr(), B, r, ROBOT_RADIUS, d_off.data_ptr(), d_idx.data_ptr(),
                                  d_cost.data_ptr(), d_ho.data_ptr(), d_hi.data_ptr(), cap, d_need.data_ptr(),
                                  d_ni.data_ptr(), d_nd.data_ptr(), None)
        ctx.sync()
        assert ctx.get_option(_capi.RRTX_OPT_LAST_PLACEMENT) == 2
        k = int(d_need.item())
        assert k == len(ref["idx"])
        got = dict(offsets=d_off.cpu().numpy(), idx=d_idx.cpu().numpy()[:k], cost=d_cost.cpu().numpy()[:k],
                   hit_out=d_ho.cpu().numpy()[:k], hit_in=d_hi.cpu().numpy()[:k], nearest_idx=d_ni.cpu().numpy(),
                   nearest_dist=d_nd.cpu().numpy())
    oracle.assert_same_results(got, ref, tuple(f for f in EXTEND_FIELDS if f != "sample_unsafe"),
                               label="null sample_unsafe: ")
