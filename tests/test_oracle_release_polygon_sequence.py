"""The contract of rrtx_obstacle_release_polygon_batch against the reference's own order, on the CPU oracle alone.  The
reference runs removeObstacle one obstacle at a time (remove A, unblock, mark A unused, remove B, ...: R/DRRT.jl:3202-3290
with :3287); the burst takes the leaving obstacles as gone together.  While A is removed B still counts as in use, so an
edge both block waits for B's turn -- and is freed there only if its start node is in B's node list.  Hence the union of
the sequence's rows is a subset of the burst's, and the two are equal when no mirrored edge is longer than delta (an edge
no longer than delta that collides with B starts within robotRadius + delta + B.radius of B's centre: it is in B's list).
Scene: the rand_Disc_3 polygons of test_gpu_obstacle_sweep_polygon.py, every colliding edge blocked."""
import numpy as np
import pytest

import release_polygon_model as M
from release_polygon_model import DELTA


@pytest.fixture(scope="module")
def scene(oracle):
    s = M.simple_scene(oracle)
    s.add = s.add_rows(oracle, range(s.m))
    s.blocked = np.unique(np.concatenate(list(s.add.values())))
    s.leaving = np.random.default_rng(40).permutation(s.m)[:40].astype(np.int32)
    return s


def _union(rows):
    return np.unique(np.concatenate(rows + [np.zeros(0, np.int32)]))


def test_the_sequence_frees_a_subset_of_what_the_burst_frees(oracle, scene):
    s = scene
    assert s.m == 89 and len(s.pts) == 2500 and int((s.length > DELTA).sum()) > 100 and len(s.blocked) > 20_000
    dist0 = np.ones(len(s.es))
    dist = dist0.copy()
    dist[s.blocked] = np.inf
    burst = s.burst_rows(oracle, s.leaving, dist)
    seq = s.sequence_rows(oracle, s.leaving, dist, dist0)
    ub, us = _union(burst), _union(seq)
    print(f"burst union {len(ub)}, sequence union {len(us)}, blocked {len(s.blocked)}, edges {len(s.es)}")
    assert len(ub) > 5000 and np.isin(us, ub).all()
    # what the sequence misses is longer than delta, and collides with a leaving obstacle whose node list lacks its start
    for e in np.setdiff1d(ub, us):
        assert s.length[e] > DELTA
        assert any(e in s.add[int(p)] for p in s.leaving) and any(
            s.active[p] and not s.mask(oracle, int(p))[s.es[e]] and oracle.explicit_edge_check_obstacle(
                s.ps, int(p), s.pts[s.es[e]], s.pts[s.ee[e]], M.RR, False) for p in s.leaving)
    # the burst is not the union of independent single removals either: edges two leaving obstacles hold come back, and
    # edges a staying obstacle holds do not
    counts = np.bincount(np.concatenate(burst), minlength=len(s.es))
    assert (counts >= 2).sum() > 100
    assert len(np.setdiff1d(s.blocked, ub)) > 1000
    single = [oracle.sweep_edges_batch(s.pts, s.es, s.ee, s.mask(oracle, int(p)), s.ps, int(p), M.RR, remove=True, dist=dist)
              for p in s.leaving]
    assert len(_union(single)) < len(ub)


def test_on_a_mirror_without_long_edges_the_two_are_equal(oracle, scene):
    s = scene
    keep = np.flatnonzero(s.length <= DELTA)
    assert 0 < len(s.es) - len(keep) < len(s.es) // 100
    short = M.make_scene(oracle, s.pts, s.tree, s.es[keep], s.ee[keep], s.polys, s.active)
    add = short.add_rows(oracle, range(s.m))
    blocked = np.unique(np.concatenate(list(add.values())))
    dist0 = np.ones(len(keep))
    dist = dist0.copy()
    dist[blocked] = np.inf
    burst = short.burst_rows(oracle, s.leaving, dist)
    seq = short.sequence_rows(oracle, s.leaving, dist, dist0)
    assert len(_union(burst)) > 5000 and np.array_equal(_union(burst), _union(seq))
    # row by row they differ (the sequence hands a shared edge to the LAST of its obstacles only)
    assert any(not np.array_equal(a, b) for a, b in zip(burst, seq))
