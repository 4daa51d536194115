"""The lattice scenes of tools/soak_lattice_sweeps.py, judged on the oracle and in exact integer arithmetic alone, with no
device involved: a lattice scene proves nothing about the obstacle sweeps and releases unless its boundary cases change
the answer.  So this file asserts, per scene, that non-root nodes sit exactly on an obstacle's range, that rows differ
when the range is bumped upward (what a `<=` in a mark kernel would return), one of them at index 63 of the batch (the
last bit of the first 64-obstacle word) and one in the second word, that mirrored edges are exactly tangent to an
inflated sphere, lie along polygon sides, pass through vertices or keep exactly the robot's radius from a side, that the
root lies exactly on a range and its out-edges leave the row one step below it, and that the release meets tangent
edges, frees some and holds some back.  tests/test_gpu_lattice_sweeps.py compares the same scenes on the device; a
change of seed or recipe that makes them insensitive fails here.

Counts of the scenes as built (seeds 7 / 7 / 5):
  S: 2950 nodes, 20 650 edges, 24 246 ids; 100 non-root nodes on a range; 21 rows change; 398 tangent edges in 35 rows;
     release: 6847 edges pass conditions 1-3, 2403 freed, 4444 held back, 146 tangent to a sphere that stays.
  P: 1885 nodes, 11 310 edges, 39 823 ids; 182 non-root nodes on a range; 45 rows change.
  D: 308 nodes, 1540 edges, 2562 ids; 12 planted nodes on their ranges; all 3 rows of the origin's boxes change."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "soak_lattice_sweeps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "soak_lattice_sweeps.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

SEED_S, SEED_P, SEED_D = 7, 7, 5


def _index_63_and_second_word(c):
    """rows that change with the range at index 63 of the batch and in the second word -- and among them rows whose
    threshold IS range^2 (le_sensitive), so that `s <= thr_lt` in a mark kernel, not only a threshold from the wrong
    side, returns other ids"""
    for key in ("changed_batch_index", "changed_le_batch_index"):
        assert 63 in c[key], f"{key}: no row that changes with the range sits at index 63 of the batch"
        assert any(i >= 64 for i in c[key]), f"{key}: no row that changes with the range sits in the second word"
    assert c["rows_changed_le"] >= 5


def _root_on_range(c, at_least):
    assert c["root_on_range"]
    assert len(c["root_row"]) >= at_least and len(c["root_row_dn"]) == 0      # the root's out-edges: in the row, gone below


def test_which_ranges_have_their_threshold_on_the_lattice():
    """thr_first_ge(r) == r * r for 3.25 and 3.75 (and the boxes' 1.875, 2.875, 3.75), one ulp below for 1.25 and 2.5"""
    assert [T.le_sensitive(r) for r in T.RANGES] == [False, False, True, True]
    assert [T.le_sensitive(r) for r in (1.875, 2.875)] == [True, True]
    assert T.thr_first_ge(1.25) == np.nextafter(1.5625, 0.0) and T.thr_first_ge(3.25) == 10.5625


def test_sphere_scene_sits_on_the_thresholds(oracle):
    s = T.sphere_scene(SEED_S)
    c = T.sphere_conditions(s)
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items()})
    assert 2800 <= c["nodes"] <= 3000 and c["edges"] == 7 * c["nodes"] and s.K == 70
    assert c["edges"] > 20 * 1024 and c["edges"] % 1024 != 0                  # several blocks of 1024 and a ragged last one
    assert (s.es[:7] == 0).all() and s.ee[7] == s.es[7] and (s.active == 0).sum() == 1
    assert set(s.search.tolist()) <= set(T.RANGES) and len(np.unique(s.order)) == 70
    assert c["on_range"] >= 50
    assert c["rows_changed_up"] >= 10
    _index_63_and_second_word(c)
    assert c["tangent_edges"] >= 50 and c["tangent_rows"] >= 10
    _root_on_range(c, 5)
    # the release: the blocked set is the union of the sweep rows of positions 0 .. 39
    assert np.array_equal(s.blocked, np.unique(np.concatenate(s.rows[:40])))
    assert len(s.leaving) == 66 and c["leaving_has_63"] and len(c["leaving_second"]) >= 1
    assert c["release_row_63"] > 0 and c["release_rows_second"] > 0           # entries 63 and 64 .. 65 free something
    assert c["release_tangent_to_staying"] >= 5
    assert c["release_freed"] >= 5 and c["release_held"] >= 5


def test_polygon_scene_sits_on_the_thresholds(oracle):
    s = T.polygon_scene(SEED_P)
    c = T.polygon_conditions(s)
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items()})
    assert 1800 <= c["nodes"] <= 2000 and c["edges"] == 6 * c["nodes"] and s.K == 70
    assert s.is_box.sum() >= 50 and set(s.kinds) == {1, 3} and (s.active == 0).sum() == 2
    assert (s.pts[:, 2] == 0.0).all() and s.rr == 0.5 and s.delta == 0.75
    assert c["on_range"] >= 100
    assert c["rows_changed_up"] >= 10
    _index_63_and_second_word(c)
    assert c["special_edges"] >= 20
    assert c["edges_along_a_side"] >= 1 and c["edges_through_a_vertex"] >= 1 and c["edges_at_rr_from_a_side"] >= 1
    _root_on_range(c, 1)
    assert c["removed_ids"] >= 20                                            # mode 1 frees something to compare


@pytest.mark.parametrize("root_planted", [False, True])
def test_dubins_scene_sits_on_the_thresholds(oracle, root_planted):
    s = T.dubins_scene(SEED_D, root_planted=root_planted)
    c = T.dubins_conditions(s)                                               # asserts every planted node itself
    print(c)
    assert c["planted"] == 4 * len(T.ORIGIN_BOXES) and c["planted_on_range"] == c["planted"]
    assert c["root_is_planted"] == root_planted
    assert c["rows_changed_up"] >= 1                                         # a planted node's out-edges cross its polygon
    th = s.pts[:, 3]
    assert (th == 0.0).any() and (th == 2.0 * np.pi).any() and s.r_min in (0.5, 1.0, 2.0)
    assert len(s.order) == 70 and set(s.order.tolist()) == set(range(s.m))
