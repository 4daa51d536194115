"""The reference the GPU tests of rrtx_extend_candidates_self_dubins compare against
(tests/extend_self_dubins_model.py), held to a plain numpy all-pairs restatement of the ghost rule -- sets and keys with
== -- and the scenes held to the cases they are there for.  No GPU."""
import numpy as np
import pytest

import extend_self_dubins_model as M


def _same_lists(ref, Q, r, wraps=M.THETA):
    j, i, key, slot, reach = M.all_pairs(Q, r, wraps)
    assert np.array_equal(np.diff(ref["offsets"]), np.bincount(j, minlength=len(Q)))
    assert np.array_equal(ref["idx"], i)                         # np.nonzero is row-major: rows in order, i ascending
    owner = np.repeat(np.arange(len(Q)), np.diff(ref["offsets"]))
    assert np.array_equal(owner, j)
    assert np.array_equal(ref["key"].view(np.uint64), key.view(np.uint64))
    return j, i, key, slot, reach


def _flags(ref, label, with_time):
    for f in ("hit_out", "hit_in"):
        free = float((ref[f] == 0).mean())
        print(f"{label}: {len(ref['idx'])} entries, {f} free {free:.3f}")
        assert 0.05 <= free <= 0.95
    values = set(ref["hit_out"].tolist()) | set(ref["hit_in"].tolist())
    assert values == ({0, 1, 2, 3} if with_time else {0, 1}), values


@pytest.mark.parametrize("name,entries", [("large", 5000), ("mid", 800), ("small", 150)])
def test_random_scenes(oracle, name, entries):
    Q, ref = M.scene(name)
    r = M.RANDOM[name][2]
    assert (Q[:, 3] >= 0.0).all() and (Q[:, 3] < M.TWO_PI).all()
    j, i, key, slot, reach = _same_lists(ref, Q, r)
    assert len(i) >= entries
    ghost = int((slot > 0).sum())
    print(f"{name}: {ghost} of {len(i)} entries found by a ghost")
    assert ghost >= 10
    _flags(ref, name, False)
    if name == "large":
        # r > pi: pairs that the sample and its ghost both reach exist, and their key is the sample's (slot 0)
        assert r > np.pi
        both = reach[0] & reach[1]
        print(f"{name}: {int(both.sum())} pairs both copies reach")
        assert both.sum() > 0 and (slot[both] == 0).all()
        d = Q[j[both]] - Q[i[both]]
        s = d[:, 0] * d[:, 0]
        s = s + d[:, 1] * d[:, 1]
        s = s + d[:, 2] * d[:, 2]
        s = s + d[:, 3] * d[:, 3]
        assert np.array_equal(ref["key"][both], np.sqrt(s))


@pytest.mark.parametrize("mode", ["time", "moving"])
@pytest.mark.parametrize("name", sorted(set(M.TIME_SIZES.values())))
def test_scenes_with_time(oracle, name, mode):
    Q, ref = M.scene(name, mode)
    flat = M.scene(name)[1]
    for k in ("offsets", "idx", "key"):                           # the lists are the search's: time changes the edges only
        assert np.array_equal(ref[k], flat[k])
    assert not np.array_equal(ref["cost_out"], flat["cost_out"])
    _flags(ref, f"{name} {mode}", True)
    if mode == "moving":
        polys, kinds, paths = M.polygon_args(name, mode)
        assert {6, 7, 3} <= set(kinds) and sum(p is not None for p in paths) == 6
        # the obstacles move: the flags differ from the static scene's
        assert not np.array_equal(ref["hit_out"], M.scene(name, "time")[1]["hit_out"])


@pytest.mark.parametrize("r", M.LATTICE_R)
def test_lattice_scenes_hold_the_boundary_cases(oracle, r):
    Q, ref = M.scene("lattice", "flat", r)
    assert len(Q) == 600 and np.array_equal(Q * 4.0, np.round(Q * 4.0)) and np.abs(Q[:, :3]).max() <= 4.0
    j, i, key, slot, reach = _same_lists(ref, Q, r)
    d = Q[:, None, :] - Q[None, :, :]
    s = (d * d).sum(axis=2)                                       # exact on this lattice, in any order
    lower = np.tril(np.ones((600, 600), dtype=bool), k=-1)
    at_r = lower & (s == r * r)                                   # sqrt(r * r) == r
    print(f"r = {r}: {int(at_r.sum())} earlier-pairs at distance exactly r, {len(i)} entries, {int((slot > 0).sum())} by a ghost")
    assert at_r.sum() >= 50
    listed = np.zeros((600, 600), dtype=bool)
    listed[j, i] = True
    # KDdist < r: a pair at exactly r is no neighbour.  (Only the ghost of the later sample can still reach such a
    # pair, and only when the two are more than 2 pi - r apart in theta: then the entry is the ghost's.)
    far = np.abs(d[..., 3]) > M.TWO_PI - r
    assert (at_r & ~far).sum() >= 50 and not (listed & at_r & ~far).any()
    by_slot = np.zeros((600, 600), dtype=int)
    by_slot[j, i] = slot
    assert (by_slot[listed & at_r] > 0).all()
    zero = lower & (s == 0.0)
    assert zero.sum() >= 3 and listed[zero].all()
    assert (key[s[j, i] == 0.0] == 0.0).all() and (slot[s[j, i] == 0.0] == 0).all()
    assert (slot > 0).sum() >= 10
    _flags(ref, f"lattice {r}", False)


@pytest.mark.parametrize("name", sorted(M.TWO_WRAPS))
def test_two_wrapped_dimensions(oracle, name):
    Q, ref = M.scene(name)
    wraps = M.TWO_WRAPS[name]
    j, i, key, slot, reach = _same_lists(ref, Q, M.RANDOM["mid"][2], wraps)
    assert {1, 2, 3} <= set(slot.tolist()) or {1, 2} <= set(slot.tolist())
    print(f"{name}: entries by slot {np.bincount(slot, minlength=4).tolist()}")
    assert (slot > 0).sum() >= 10
    _flags(ref, name, False)
    # the order of set_wrap renumbers the copies and changes no list
    other = M.scene([n for n in M.TWO_WRAPS if n != name][0])[1]
    for k in ("offsets", "idx", "key", "cost_out", "hit_out"):
        assert np.array_equal(ref[k], other[k])


def test_no_wrapped_dimension(oracle):
    Q, ref = M.scene("nowrap")
    j, i, key, slot, reach = _same_lists(ref, Q, M.RANDOM["mid"][2], ((), ()))
    assert (slot == 0).all() and len(i) >= 800
    wrapped = M.scene("mid")[1]
    assert len(wrapped["idx"]) > len(i)                            # the ghosts of the wrapped scene add entries
    _flags(ref, "nowrap", False)


def test_skip_takes_a_sample_out_of_every_list(oracle):
    O = oracle
    Q, ref = M.scene("mid")
    skip = np.random.default_rng(5).random(len(Q)) < 1.0 / 3.0
    polys, kinds, paths = M.polygon_args("mid", "flat")
    got = M.self_reference(O, Q, M.RANDOM["mid"][2], O.PolygonSet(polys, kinds=kinds, paths=paths), skip=skip)
    owner = np.repeat(np.arange(len(Q)), np.diff(ref["offsets"]))
    keep = ~skip[owner] & ~skip[ref["idx"]]
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(np.diff(got["offsets"]), np.bincount(owner[keep], minlength=len(Q)))
    for k in ("idx", "key", "cost_out", "cost_in", "word_out", "word_in", "hit_out", "hit_in"):
        assert np.array_equal(got[k], ref[k][keep])


def test_a_prefix_of_a_batch_has_the_first_rows(oracle):
    O = oracle
    Q, ref = M.scene("small")
    polys, kinds, paths = M.polygon_args("small", "flat")
    for b in (1, 2, 63, 64):
        got = M.self_reference(O, Q[:b], M.RANDOM["small"][2], O.PolygonSet(polys, kinds=kinds, paths=paths))
        want = M.prefix(ref, b)
        for k in ("offsets", "idx", "key", "cost_out", "cost_in", "word_out", "word_in", "hit_out", "hit_in"):
            assert np.array_equal(got[k], want[k])
