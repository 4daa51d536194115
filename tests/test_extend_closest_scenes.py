"""The reference the GPU tests of rrtx_extend_closest_self compare against (tests/extend_closest_model.py), held to the
oracle's kdFindNearest over the earlier live samples, and the scenes held to the cases they are there for.  No GPU."""
import numpy as np
import pytest

import extend_closest_model as M
import extend_self_model as S


def _first_entry_is_kd_nearest(oracle, Q, ref, skip=None, want=None):
    """the samples go into the reference's kd-tree one after the other (the live ones): before sample j goes in, the
    distance kdFindNearest gives for it is the cost of the first entry of row j"""
    live = M.live_samples(Q, skip)
    tree, n = oracle.KDTree(3), 0
    for j in range(len(Q)):
        filled = live[j] and (want is None or want[j])
        if filled and n > 0:
            _, dist = tree.nearest(Q[j])
            assert ref["count"][j] >= 1
            assert np.float64(dist).view(np.uint64) == ref["cost"][j, 0].view(np.uint64), j
        else:
            assert ref["count"][j] == 0 and ref["idx"][j, 0] == -1 and ref["cost"][j, 0] == np.inf
        if live[j]:
            tree.insert(Q[j])
            n += 1


def _well_formed(Q, ref, k):
    """rows sorted by (cost, idx), indices below the row, unused slots -1 / +Inf / 0"""
    for j in range(len(Q)):
        n = int(ref["count"][j])
        assert 0 <= n <= min(k, j)
        i, c = ref["idx"][j], ref["cost"][j]
        assert (i[:n] >= 0).all() and (i[:n] < j).all() and len(set(i[:n])) == n
        assert (i[n:] == -1).all() and (c[n:] == np.inf).all()
        assert not ref["hit_out"][j, n:].any() and not ref["hit_in"][j, n:].any()
        key = list(zip(c[:n], i[:n]))
        assert key == sorted(key)


def test_lattice_scene_holds_ties_and_duplicates(oracle):
    Q, ref = M.scene("spheres", "lattice")
    assert len(Q) == 600 and np.array_equal(Q * 4.0, np.round(Q * 4.0))
    _well_formed(Q, ref, M.MAX_K)
    _first_entry_is_kd_nearest(oracle, Q, ref)
    rows = M.ranked_rows(Q)
    for k in (1, 2, 8, 32):
        # ties on s at the k-th place: the k-th and the (k+1)-th candidate at the same distance, the lower index kept
        tied = [j for j, (i, s) in enumerate(rows) if len(i) > k and s[k - 1] == s[k]]
        print(f"k = {k}: {len(tied)} rows with a tie at the k-th place")
        assert len(tied) >= 5
        for j in tied[:5]:
            i, _ = rows[j]
            assert i[k - 1] < i[k] and ref["idx"][j, k - 1] == i[k - 1]
    zero = (ref["cost"] == 0.0) & (ref["idx"] >= 0)
    assert zero.sum() >= 3                                          # pairs at distance 0 (the planted duplicates)
    # a zero-length edge collides with every sphere in use
    assert ref["hit_out"][zero].all() and ref["hit_in"][zero].all()
    for a, b in S.DUPLICATES:
        assert ref["idx"][a, 0] == b and ref["cost"][a, 0] == 0.0


@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_rows_shorter_than_exactly_and_longer_than_k(oracle, k):
    Q, full = M.scene("spheres", "small")
    ref = M.narrow(full, len(Q), k)
    _well_formed(Q, ref, k)
    earlier = np.arange(len(Q))                                     # every sample of the scene is live
    assert (ref["count"][earlier < k] == earlier[earlier < k]).all()    # fewer than k
    assert ref["count"][k] == k                                     # exactly k
    assert (ref["count"][earlier > k] == k).all() and (earlier > k).sum() >= 30
    # the narrowed reference is the reference computed for k
    own = M.closest_reference(oracle, Q, k, S.obstacles(oracle, "spheres", "small"))
    for f in M.FIELDS:
        assert np.array_equal(own[f], ref[f]), f


def test_a_marked_and_a_non_finite_sample_in_the_middle(oracle):
    Q, skip = M.marked_samples()
    obs = S.obstacles(oracle, "spheres", "mid")
    ref = M.closest_reference(oracle, Q, 8, obs, skip=skip)
    _well_formed(Q, ref, 8)
    _first_entry_is_kd_nearest(oracle, Q, ref, skip=skip)
    for j in (M.MARKED, M.NOT_FINITE):
        assert ref["count"][j] == 0 and not (ref["idx"] == j).any()
    clean = M.narrow(M.scene("spheres", "mid")[1], len(Q), 8)
    # ... and somebody had them among the first 8 before: the rows of the others close up
    assert (clean["idx"] == M.MARKED).any() and (clean["idx"] == M.NOT_FINITE).any()
    moved = (clean["idx"] != ref["idx"]).any(axis=1)
    assert moved[[M.MARKED, M.NOT_FINITE]].all() and 2 < moved.sum() < len(Q) // 2
    # want leaves a sample a candidate of the others
    want = (np.random.default_rng(3).random(len(Q)) < 0.5).astype(np.uint8)
    half = M.closest_reference(oracle, Q, 8, obs, skip=skip, want=want)
    _first_entry_is_kd_nearest(oracle, Q, half, skip=skip, want=want)
    for f in M.FIELDS:
        assert np.array_equal(half[f][want != 0], ref[f][want != 0]), f
    assert (half["count"][want == 0] == 0).all() and (half["idx"][want == 0] == -1).all()
    assert (want[half["idx"][half["idx"] >= 0]] == 0).any()


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_random_scenes_hold_blocked_and_free_edges(oracle, kind):
    for name in ("large", "mid", "small"):
        Q, ref = M.scene(kind, name)
        _well_formed(Q, ref, M.MAX_K)
        _first_entry_is_kd_nearest(oracle, Q, ref)
        for k in (1, 8, 32):
            used = ref["idx"][:, :k] >= 0
            for f in ("hit_out", "hit_in"):
                v = ref[f][:, :k][used]
                print(f"{kind} {name} k = {k}: {int(used.sum())} entries, {f} blocked {float(v.mean()):.3f}")
                if name != "small" or k > 1:
                    assert 0 < v.sum() < len(v)


def test_tree_column(oracle):
    Q, _ = M.scene("spheres", "mid")
    tree = S.tree_points(200)
    obs = S.obstacles(oracle, "spheres", "mid")
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    ti[5], ti[6] = -1, len(tree)
    ref = M.closest_reference(oracle, Q, 2, obs, tree_idx=ti, tree_pts=tree)
    assert ref["tree_hit_out"][5] == ref["tree_hit_out"][6] == ref["tree_hit_in"][5] == ref["tree_hit_in"][6] == 0
    for f in M.TREE_FIELDS:
        assert 0 < ref[f].sum() < len(Q), f
    # row 0 has no earlier sample and still has its tree column
    assert ref["count"][0] == 0
    h, _ = oracle.edges_check_batch(obs, Q[:1], tree[ti[:1]], M.RR)
    assert ref["tree_hit_out"][0] == h[0]
