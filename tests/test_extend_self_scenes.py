"""The reference the GPU tests of rrtx_extend_candidates_self compare against (tests/extend_self_model.py), held to a
plain numpy all-pairs count, and the scenes held to the cases they are there for.  No GPU."""
import numpy as np
import pytest

import extend_self_model as M


def _same_lists(ref, Q, r):
    j, i, s = M.all_pairs(Q, r)
    assert np.array_equal(np.diff(ref["offsets"]), np.bincount(j, minlength=len(Q)))
    assert np.array_equal(ref["idx"], i)                         # np.nonzero is row-major: rows in order, i ascending
    owner = np.repeat(np.arange(len(Q)), np.diff(ref["offsets"]))
    assert np.array_equal(owner, j)
    assert np.array_equal(ref["cost"].view(np.uint64), np.sqrt(s[j, i]).view(np.uint64))
    # one value serves as the key of the range search and as the SimpleEdge cost in either direction
    assert np.array_equal(ref["cost"].view(np.uint64), ref["key"].view(np.uint64))
    assert np.array_equal(ref["cost"].view(np.uint64), ref["cost_in"].view(np.uint64))
    return j, i, s


@pytest.mark.parametrize("r", M.LATTICE_R)
def test_lattice_scenes_hold_the_boundary_cases(oracle, r):
    Q, ref = M.scene("spheres", "lattice", r)
    assert len(Q) == 600 and np.array_equal(Q * 4.0, np.round(Q * 4.0)) and np.abs(Q).max() <= 4.0
    j, i, s = _same_lists(ref, Q, r)
    lower = np.tril(np.ones((600, 600), dtype=bool), k=-1)
    at_r = lower & (s == r * r)                                  # exact on this lattice; sqrt(r * r) == r
    assert at_r.sum() >= 100
    print(f"r = {r}: {int(at_r.sum())} earlier-pairs at distance exactly r, {len(i)} entries")
    listed = np.zeros((600, 600), dtype=bool)
    listed[j, i] = True
    assert not (listed & at_r).any()                             # KDdist < r: a pair at exactly r is no neighbour
    zero = lower & (s == 0.0)
    assert zero.sum() >= 3 and listed[zero].all()
    assert (ref["cost"][s[j, i] == 0.0] == 0.0).all()
    # a zero-length edge collides with every sphere in use
    assert (ref["hit_out"][s[j, i] == 0.0] == 1).all() and (ref["hit_in"][s[j, i] == 0.0] == 1).all()
    counts = np.diff(ref["offsets"])
    assert counts[0] == 0 and (counts[1:] == 0).sum() >= 1      # empty rows beside the first


@pytest.mark.parametrize("kind", ["spheres", "polygons"])
def test_random_scenes_hold_blocked_and_free_edges(oracle, kind):
    differ = 0
    for name, entries in (("large", 5000), ("mid", 800), ("small", 150)):
        Q, ref = M.scene(kind, name)
        _same_lists(ref, Q, M.RANDOM[name][2])
        n = len(ref["idx"])
        assert n >= entries
        for f in ("hit_out", "hit_in"):
            blocked = float(ref[f].mean())
            print(f"{kind} {name}: {n} entries, {f} blocked {blocked:.3f}")
            assert 0.05 <= blocked <= 0.95
        differ += int((ref["hit_out"] != ref["hit_in"]).sum())
    print(f"{kind}: {differ} entries whose two flags differ")
    if kind == "spheres":
        assert differ >= 1


def test_skip_takes_a_sample_out_of_every_list(oracle):
    Q, ref = M.scene("spheres", "mid")
    skip = np.random.default_rng(5).random(len(Q)) < 1.0 / 3.0
    got = M.self_reference(oracle, Q, M.RANDOM["mid"][2], M.obstacles(oracle, "spheres", "mid"), skip=skip)
    owner = np.repeat(np.arange(len(Q)), np.diff(ref["offsets"]))
    keep = ~skip[owner] & ~skip[ref["idx"]]
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(np.diff(got["offsets"]), np.bincount(owner[keep], minlength=len(Q)))
    for k in ("idx", "cost", "hit_out", "hit_in"):
        assert np.array_equal(got[k], ref[k][keep])


def test_a_prefix_of_a_batch_has_the_first_rows(oracle):
    Q, ref = M.scene("spheres", "small")
    for b in (1, 2, 63, 64):
        got = M.self_reference(oracle, Q[:b], M.RANDOM["small"][2], M.obstacles(oracle, "spheres", "small"))
        want = M.prefix(ref, b)
        for k in ("offsets", "idx", "cost", "hit_out", "hit_in"):
            assert np.array_equal(got[k], want[k])
