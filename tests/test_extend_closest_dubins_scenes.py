"""The reference the GPU tests of rrtx_extend_closest_self_dubins compare against
(tests/extend_closest_dubins_model.py), held to the oracle's kdFindNearest in the wrapped space over the earlier live
samples, and the scenes held to the cases they are there for.  No GPU."""
import numpy as np
import pytest

import extend_closest_dubins_model as M
import extend_self_dubins_model as S


def _first_entry_is_kd_nearest(oracle, Q, ref, wraps, skip=None, want=None):
    """the samples go into the reference's kd-tree one after the other (the live ones): before sample j goes in, the
    distance kdFindNearest gives for it is the key of the first entry of row j, and its index wherever no other earlier
    sample is at that distance.  Returns the number of rows compared and of unique minima."""
    live = M.live_samples(Q, skip)
    tree = oracle.KDTree(4, list(wraps[0]), list(wraps[1])) if wraps[0] else oracle.KDTree(4)
    node_of, rows, unique = [], 0, 0
    s, _ = M.s_all(np.where(np.isfinite(Q), Q, 0.0), wraps)
    for j in range(len(Q)):
        filled = live[j] and (want is None or want[j])
        if filled and node_of:
            idx, dist = tree.nearest(Q[j])
            assert ref["count"][j] >= 1
            assert np.float64(dist).view(np.uint64) == ref["key"][j, 0].view(np.uint64), j
            rows += 1
            earlier = np.asarray(node_of)
            if (s[j, earlier] == s[j, ref["idx"][j, 0]]).sum() == 1:
                assert node_of[idx] == ref["idx"][j, 0], j
                unique += 1
        else:
            assert ref["count"][j] == 0 and ref["idx"][j, 0] == -1 and ref["key"][j, 0] == np.inf
        if live[j]:
            tree.insert(Q[j])
            node_of.append(j)
    return rows, unique


def _well_formed(Q, ref, k):
    """rows sorted by (key, idx), indices below the row, unused slots -1 / +Inf / no word / 0"""
    for j in range(len(Q)):
        n = int(ref["count"][j])
        assert 0 <= n <= min(k, j)
        i, c = ref["idx"][j], ref["key"][j]
        assert (i[:n] >= 0).all() and (i[:n] < j).all() and len(set(i[:n])) == n
        assert (i[n:] == -1).all() and (c[n:] == np.inf).all()
        assert (ref["cost_out"][j, n:] == np.inf).all() and (ref["cost_in"][j, n:] == np.inf).all()
        assert (ref["word_out"][j, n:] == M.NO_WORD).all() and (ref["word_in"][j, n:] == M.NO_WORD).all()
        assert not ref["hit_out"][j, n:].any() and not ref["hit_in"][j, n:].any()
        key = list(zip(c[:n], i[:n]))
        assert key == sorted(key)


@pytest.mark.parametrize("name,most", [("mid", 1), ("theta_t", 3), ("t_theta", 3), ("three", 7), ("nowrap", 0)])
def test_first_entry_is_kd_nearest_and_ghosts_attain_minima(oracle, name, most):
    """one, two (both orders of rrtx_set_wrap) and three wrapped dimensions, and none: rows whose first entry's minimum is
    attained by a ghost and not by the sample itself exist for every slot there is"""
    Q, ref, wraps = M.scene(name)
    assert len(wraps[0]) == {0: 0, 1: 1, 3: 2, 7: 3}[most]
    _well_formed(Q, ref, M.MAX_K)
    rows, unique = _first_entry_is_kd_nearest(oracle, Q, ref, wraps)
    assert rows == len(Q) - 1 and unique >= rows - 2
    rk = M.ranked_rows(Q, wraps)
    slots = np.array([r[2][0] for r in rk[1:]])
    print(f"{name}: first entry by slot {np.bincount(slots, minlength=most + 1).tolist()}")
    # first entries: the sample itself, every single shift, and with more than one wrap a double shift; among the first
    # MAX_K entries of the rows every slot attains a minimum
    assert set(slots.tolist()) >= {0} | {1 << n for n in range(len(wraps[0]))}
    assert most < 3 or (np.bincount(slots, minlength=8)[[3, 5, 6]] > 0).any()
    deep = np.concatenate([r[2][:M.MAX_K] for r in rk[1:]])
    print(f"{name}: entries by slot {np.bincount(deep, minlength=most + 1).tolist()}")
    assert set(deep.tolist()) == set(range(most + 1))
    assert (slots != 0).sum() >= (10 if most else 0)
    # the ghost matters: with the sample's own copy alone the first entry would be another or farther away
    if most:
        own = M.ranked_rows(Q, ((), ()))
        worse = sum(1 for a, b in zip(rk[1:], own[1:]) if a[1][0] < b[1][0])
        assert worse >= 10
    if name in S.TWO_WRAPS:
        # the two orders name the same space: the rows agree although the slots are numbered the other way round
        other = M.scene({"theta_t": "t_theta", "t_theta": "theta_t"}[name])[1]
        assert np.array_equal(other["idx"], ref["idx"]) and np.array_equal(other["key"], ref["key"])


def test_lattice_scene_holds_ties_and_duplicates(oracle):
    Q, ref, wraps = M.scene("lattice")
    assert len(Q) == 600 and np.array_equal(Q * 4.0, np.round(Q * 4.0))
    _well_formed(Q, ref, M.MAX_K)
    rows, unique = _first_entry_is_kd_nearest(oracle, Q, ref, wraps)
    assert rows == 599 and 0 < unique < rows            # first places are tied as well
    rk = M.ranked_rows(Q, wraps)
    for k in (1, 2, 8, 32):
        # ties on s at the k-th place: the k-th and the (k+1)-th candidate at the same distance, the lower index kept
        tied = [j for j, (i, s, _) in enumerate(rk) if len(i) > k and s[k - 1] == s[k]]
        print(f"k = {k}: {len(tied)} rows with a tie at the k-th place")
        assert len(tied) >= 5
        for j in tied[:5]:
            i = rk[j][0]
            assert i[k - 1] < i[k] and ref["idx"][j, k - 1] == i[k - 1]
    zero = (ref["key"] == 0.0) & (ref["idx"] >= 0)
    assert zero.sum() >= 3                                          # pairs at distance 0 (the planted duplicates)
    for a, b in S.DUPLICATES:
        assert ref["idx"][a, 0] == b and ref["key"][a, 0] == 0.0
    # a ghost on the lattice: theta is a multiple of 1/4 but the period is not, so a ghost's distance ties with nothing
    assert any(r[2][0] == 1 for r in rk[1:])


@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_rows_shorter_than_exactly_and_longer_than_k(oracle, k):
    Q, full, wraps = M.scene("small")
    ref = M.narrow(full, len(Q), k)
    _well_formed(Q, ref, k)
    earlier = np.arange(len(Q))                                     # every sample of the scene is live
    assert (ref["count"][earlier < k] == earlier[earlier < k]).all()    # fewer than k
    assert ref["count"][k] == k                                     # exactly k
    assert (ref["count"][earlier > k] == k).all() and (earlier > k).sum() >= 30
    # the narrowed reference is the reference computed for k
    own = M.closest_reference(oracle, Q, k, M.polygon_set(oracle, "small"), wraps=wraps)
    for f in M.FIELDS:
        assert np.array_equal(own[f], ref[f]), f


def test_a_marked_and_a_non_finite_sample_in_the_middle(oracle):
    Q, skip = M.marked_samples()
    ps = M.polygon_set(oracle, "mid")
    ref = M.closest_reference(oracle, Q, 8, ps, skip=skip)
    _well_formed(Q, ref, 8)
    _first_entry_is_kd_nearest(oracle, Q, ref, S.THETA, skip=skip)
    for j in (M.MARKED, M.NOT_FINITE):
        assert ref["count"][j] == 0 and not (ref["idx"] == j).any()
    clean = M.narrow(M.scene("mid")[1], len(Q), 8)
    # ... and somebody had them among the first 8 before: the rows of the others close up
    assert (clean["idx"] == M.MARKED).any() and (clean["idx"] == M.NOT_FINITE).any()
    moved = (clean["idx"] != ref["idx"]).any(axis=1)
    assert moved[[M.MARKED, M.NOT_FINITE]].all() and 2 < moved.sum() < len(Q) // 2
    # want leaves a sample a candidate of the others
    want = (np.random.default_rng(3).random(len(Q)) < 0.5).astype(np.uint8)
    half = M.closest_reference(oracle, Q, 8, ps, skip=skip, want=want)
    _first_entry_is_kd_nearest(oracle, Q, half, S.THETA, skip=skip, want=want)
    for f in M.FIELDS:
        assert np.array_equal(half[f][want != 0], ref[f][want != 0]), f
    assert (half["count"][want == 0] == 0).all() and (half["idx"][want == 0] == -1).all()
    assert (want[half["idx"][half["idx"] >= 0]] == 0).any()


@pytest.mark.parametrize("name", ["large", "mid", "small", "theta_t", "three", "nowrap", "lattice"])
def test_scenes_hold_blocked_and_free_edges(oracle, name):
    """free and blocked entries both above 5 % of the entries, in either direction"""
    Q, ref, _ = M.scene(name)
    for k in (1, 8, 32):
        used = ref["idx"][:, :k] >= 0
        for f in ("hit_out", "hit_in"):
            v = ref[f][:, :k][used]
            print(f"{name} k = {k}: {int(used.sum())} entries, {f} blocked {float(v.mean()):.3f}")
            assert set(v.tolist()) <= {0, 1}
            assert 0.05 < v.mean() < 0.95


@pytest.mark.parametrize("mode", ["time", "moving"])
@pytest.mark.parametrize("name", ["small", "mid"])
def test_scenes_with_time_hold_every_flag_value(oracle, name, mode):
    Q, ref, wraps = M.scene(name, mode)
    _well_formed(Q, ref, M.MAX_K)
    for k in (1, 8, 32):
        used = ref["idx"][:, :k] >= 0
        for f in ("hit_out", "hit_in"):
            v = ref[f][:, :k][used]
            share = np.bincount(v, minlength=4) / len(v)
            print(f"{name} {mode} k = {k}: {f} flag values {np.round(share, 3).tolist()}")
            if k > 1:
                assert (share > 0).all() and len(share) == 4
            assert 0.05 < (v & 1).mean() < 0.95
    # the keys do not depend on the mode
    assert np.array_equal(ref["idx"], M.scene(name)[1]["idx"])


def test_tree_column(oracle):
    Q, _, wraps = M.scene("mid")
    tree = S.tree_points(200, hw=6.0)
    ps = M.polygon_set(oracle, "mid")
    ti = np.random.default_rng(8).integers(0, len(tree), len(Q)).astype(np.int32)
    ti[5], ti[6] = -1, len(tree)
    ref = M.closest_reference(oracle, Q, 2, ps, tree_idx=ti, tree_pts=tree)
    for j in (5, 6):
        assert ref["tree_cost_out"][j] == ref["tree_cost_in"][j] == np.inf
        assert ref["tree_hit_out"][j] == ref["tree_hit_in"][j] == 0 and ref["tree_word_out"][j] == M.NO_WORD
    for f in ("tree_hit_out", "tree_hit_in"):
        assert 0 < ref[f].sum() < len(Q), f
    # row 0 has no earlier sample and still has its tree column
    assert ref["count"][0] == 0
    e = oracle.dubins_edges_batch(Q[:1], tree[ti[:1]], M.RMIN, ps, M.RR)
    assert ref["tree_hit_out"][0] == e["hit"][0] and ref["tree_cost_out"][0] == e["cost"][0]
    assert ref["tree_word_out"][0] == e["word"][0]
