"""nn_finish, lists of up to 64 entries: the rank inside the half wave, the nearest of the list, the offsets and
the capacity guard, each against the CPU oracle with ==.

A list of any exact length: the nodes sit along the x axis one unit apart in a shuffled order of their indices, and a
sample half a unit in front of the line's end with radius L + 0.25 reaches the positions 0 .. L - 1 -- node indices in
shuffled order.  Two consecutive samples share a wave of nn_finish, sixteen a workgroup.  The line of 8 209 nodes
takes the culled route of the search, the one of 257 the brute-force scan; both end in this kernel."""
import itertools

import numpy as np
import pytest

from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
PARTNERS = (0, 16, 32, 64)
LINES = {"brute": 257, "culled": 8209}
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def line(route):
    """(node positions, oracle tree) of the line that takes `route`"""
    def make(oracle):
        n = LINES[route]
        perm = np.random.default_rng(5 + n).permutation(n)
        pos = np.arange(n)
        pts = np.zeros((n, 3))
        pts[perm, 0] = pos
        pts[perm, 1] = 0.001 * ((pos * 7919) % 97 - 48)      # less than 0.05 off the axis: the kd-tree has three
        pts[perm, 2] = 0.001 * ((pos * 104729) % 89 - 44)    # coordinates to split on
        tree = oracle.KDTree(3)
        tree.insert_many(pts)
        return pts, tree
    return lambda oracle: _once(("line", route), lambda: make(oracle))


def samples_for(lengths):
    """one sample per wanted list length: in front of the line's end, a little off the axis (no two samples equal)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    nq = len(lengths)
    Q = np.zeros((nq, 3))
    Q[:, 0] = -0.5
    Q[:, 1] = 1e-4 * (np.arange(nq) % 1000)         # <= 0.1: position p is at p + 0.5 + less than 0.03
    return Q, lengths + 0.25                          # reaches position L - 1 (L - 0.5 away), not L (L + 0.5)


def pair_lengths():
    """every length in the lower and in the upper half of a wave beside every partner length, and one odd sample"""
    out = []
    for n, p in itertools.product(LENGTHS, PARTNERS):
        out += [n, p, p, n]
    return out + [17]


def assert_lists(got, ref, label):
    off, idx, dist = got
    assert np.array_equal(off, ref["offsets"]), f"{label}: offsets"
    assert np.array_equal(idx, ref["idx"]), f"{label}: idx"
    assert np.array_equal(dist, ref["key"]), f"{label}: dist"


@pytest.mark.parametrize("route", sorted(LINES))
def test_every_length_beside_every_partner(oracle, route):
    pts, tree = line(route)(oracle)
    want = pair_lengths()
    nq = len(want)
    assert nq == 241 and nq % 16 == 1                 # a last workgroup of one sample: a wave with an invalid half
    Q, r = samples_for(want)
    ref = oracle.range_batch(tree, Q, r)
    assert np.array_equal(np.diff(ref["offsets"]), want)
    last = ref["idx"][ref["offsets"][-2]:]
    assert (np.diff(last) > 0).all() and (np.diff(pts[last, 0]) < 0).any()      # ascending indices, not positions
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        assert_lists(ctx.nn_radius(Q, r), ref, f"{route}, {nq} samples")
        Q1, r1 = samples_for([49])
        assert_lists(ctx.nn_radius(Q1, r1), oracle.range_batch(tree, Q1, r1), f"{route}, one sample")


def test_offsets_of_a_large_batch(oracle):
    """late workgroups add up thousands of preceding counts: the unrolled part and the remainder of that loop"""
    pts, tree = line("culled")(oracle)
    nq = 32_803
    j = np.arange(nq)
    Q = np.zeros((nq, 3))
    Q[:, 0] = (j * 37) % 8000 + 0.25                  # 0.25 from one node, 0.75 and 1.25 from the next two
    Q[:, 1] = 1e-6 * (j % 1000)
    r = np.array([0.1, 0.5, 1.0, 1.5])[(j * 7 + j // 5) % 4]
    trees = _once("line trees", lambda: oracle.TreeSet(3, pts))             # one tree per thread
    ref = oracle.range_batch(trees, Q, r, per_sample=4.0, nearest=False, slice_size=1024)
    counts = np.diff(ref["offsets"])
    assert np.array_equal(counts, np.array([0, 1, 2, 3])[(j * 7 + j // 5) % 4])
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        off, idx, dist = ctx.nn_radius(Q, r)
    assert np.array_equal(off[1:], np.cumsum(counts)) and off[0] == 0 and len(idx) == off[-1]
    assert_lists((off, idx, dist), ref, "large batch")


@pytest.mark.parametrize("route", sorted(LINES))
def test_capacity_smaller_than_the_need(oracle, route):
    """offsets and the count stay exact and nothing at or behind cap is written (what lies in front of cap is not
    specified for a call that reports too small a capacity: the caller repeats it with the count)"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    pts, tree = line(route)(oracle)
    R = 70.0
    want = np.array([k for pair in itertools.product(LENGTHS, PARTNERS) for k in pair] + [5])
    nq = len(want)
    Q = np.zeros((nq, 3))
    Q[:, 0] = want - 0.5 - R                           # one radius for all: the sample moves instead
    Q[:, 1] = 1e-4 * np.arange(nq)
    ref = oracle.range_batch(tree, Q, R)
    assert np.array_equal(np.diff(ref["offsets"]), want)
    need = int(ref["offsets"][-1])
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        st = torch.cuda.Stream(device=dev)
        ctx.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_q = torch.from_numpy(Q).to(dev)
            for cap in (need // 2 + 3, 40, need):
                d_off = torch.full((nq + 1,), -7, dtype=torch.int64, device=dev)
                d_idx = torch.full((need + 64,), -7, dtype=torch.int32, device=dev)
                d_dist = torch.full((need + 64,), -7.0, dtype=torch.float64, device=dev)
                d_need = torch.zeros(1, dtype=torch.int64, device=dev)
                st.synchronize()
                ctx.nn_radius_dev(d_q.data_ptr(), R, nq, d_off.data_ptr(), d_idx.data_ptr(), d_dist.data_ptr(), cap,
                                  d_need.data_ptr())
                st.synchronize()
                idx, dist = d_idx.cpu().numpy(), d_dist.cpu().numpy()
                assert int(d_need.item()) == need and np.array_equal(d_off.cpu().numpy(), ref["offsets"]), cap
                if cap == need:
                    assert np.array_equal(idx[:cap], ref["idx"]) and np.array_equal(dist[:cap], ref["key"]), cap
                assert (idx[cap:] == -7).all() and (dist[cap:] == -7.0).all(), cap
        ctx.set_stream(None)


# ---- the nearest of a list among equals ------------------------------------------------------------------------------
def _ring():
    """the 48 signed permutations of (1, 2, 3): integer points, all at squared distance 14 from the origin"""
    pts = {tuple(s * v for s, v in zip(sg, pm)) for pm in itertools.permutations((1, 2, 3))
           for sg in itertools.product((1, -1), repeat=3)}
    return np.array(sorted(pts), dtype=np.float64)


@pytest.mark.parametrize("filler", (0, 8200))
def test_nearest_among_equals_is_the_lowest_index(oracle, filler):
    ring = _ring()
    assert ring.shape == (48, 3) and ((ring ** 2).sum(axis=1) == 14.0).all()
    rng = np.random.default_rng(11)
    sizes = (48, 2, 17, 33)
    centres = np.array([[100.0 * (c + 1), 40.0, -20.0] for c in range(len(sizes))])
    groups = [centres[c] + ring[rng.permutation(48)[:k]] for c, k in enumerate(sizes)]
    far = np.zeros((filler, 3))
    far[:, 0] = 5000.0 + np.arange(filler)            # (the culled route needs 8 192 nodes)
    pts = np.concatenate(groups + [far])
    group_of = np.repeat(np.arange(len(sizes) + 1), list(sizes) + [filler])
    order = rng.permutation(len(pts))                  # node i is pts[order[i]]: every group's indices are scattered
    pts, group_of = pts[order], group_of[order]
    lone = np.array([[37.25, -11.5, 3.125]])          # an empty ball in the same workgroup: the expanding search
    Q = np.concatenate([centres, lone, centres[::-1]])
    r = 4.0                                            # 14 < 16
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    ref = oracle.range_batch(tree, Q, r)
    assert list(np.diff(ref["offsets"])) == list(sizes) + [0] + list(sizes[::-1])
    assert (ref["key"] == np.sqrt(14.0)).all()
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(np.array([[0.0, 0.0, 900.0, 1.0]]))          # far from every edge
        out = ctx.extend_candidates(Q, r, 0.5)
    assert np.array_equal(out["offsets"], ref["offsets"]) and np.array_equal(out["idx"], ref["idx"])
    assert np.array_equal(out["cost"], ref["key"]) and not out["hit_out"].any() and not out["hit_in"].any()
    for j, c in enumerate(list(range(len(sizes))) + [None] + list(range(len(sizes)))[::-1]):
        if c is None:
            assert out["nearest_idx"][j] == ref["nearest_idx"][j] and out["nearest_dist"][j] == ref["nearest_dist"][j]
        else:
            assert out["nearest_idx"][j] == np.flatnonzero(group_of == c).min(), (j, c)
            assert out["nearest_dist"][j] == np.sqrt(14.0), (j, c)


# ---- the flags of the fused extend path travel with their records -------------------------------------------------------
def test_flags_follow_their_records(oracle):
    from rrtqx_3d_amd import synth
    rng = np.random.default_rng(23)
    n, nq, rr = 9_000, 333, 0.5
    pts = rng.uniform(-10.0, 10.0, (n, 3))
    Q = rng.uniform(-9.0, 9.0, (nq, 3))
    sph = np.concatenate([rng.uniform(-10.0, 10.0, (24, 3)), rng.uniform(3.0, 4.0, (24, 1))], axis=1)
    r = 1.9                                            # about 32 neighbours a sample
    tree = oracle.KDTree(3)
    tree.insert_many(pts)
    ref = oracle.range_batch(tree, Q, r)
    counts = np.diff(ref["offsets"])
    assert (counts < 32).sum() > 50 and ((counts > 32) & (counts <= 64)).sum() > 50
    p0, p1 = synth.candidate_edges(Q, pts, ref["offsets"], ref["idx"])
    arr, m = oracle.make_spheres(sph)
    hit, _ = oracle.edges_check_spheres(arr, m, p0, p1, rr)
    k = len(ref["idx"])
    assert 0.3 < hit.mean() < 0.7
    with Context(3) as ctx:
        ctx.nodes_append(pts)
        ctx.spheres_set(sph)
        out = ctx.extend_candidates(Q, r, rr)
    assert np.array_equal(out["offsets"], ref["offsets"]) and np.array_equal(out["idx"], ref["idx"])
    assert np.array_equal(out["cost"], ref["key"])
    assert np.array_equal(out["hit_out"], hit[:k]) and np.array_equal(out["hit_in"], hit[k:])
    assert np.array_equal(out["nearest_idx"], ref["nearest_idx"]) and np.array_equal(out["nearest_dist"], ref["nearest_dist"])
