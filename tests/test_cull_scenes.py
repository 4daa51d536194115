"""What the GPU tests of rrtx_graph_edges_cull / _compact rely on, asserted on the CPU: the growth scene culls enough edges,
enough of them parent edges of the fixed point before the cull, enough nodes change rrtLMC, a blocked edge is among the
culled ones once a sphere is swept; the lattice cases hold an edge whose cost is the ball exactly; the renumbering model
is a stable compaction.  The fixed points are the oracle's (oracle.Graph, reduceInconsistency with hyberBallRad = +Inf)."""
import numpy as np
import pytest

import cull_model as CM
from mirror_model import MirrorModel
from test_gpu_cost_delta import RR, SPHERE_RADIUS, Scene as DeltaScene, _lowest_parent
from test_gpu_graph_cost import _edge_dist, _oracle_solve

INF = float("inf")
N, SEED, BALL_CONSTANT, ROOT = 2000, 5, 30.0, 0


@pytest.fixture(scope="module")
def scene():
    return CM.growth_scene(N, SEED, BALL_CONSTANT)


def test_growth_scene_culls_parent_edges_and_changes_costs(oracle, scene):
    pts, s, e, w = scene
    assert np.array_equal(w, _edge_dist(pts, s, e))              # the model's cost is the mirror's
    ball = CM.ball(N, BALL_CONSTANT)
    assert 4.6 < ball < 4.8
    m = CM.CullModel(pts, s, e)
    lmc0 = np.ascontiguousarray(_oracle_solve(oracle, N, s, e, w, ROOT)[0])
    par0 = _lowest_parent(lmc0, s, e, w, ROOT)
    ids = m.cull(ball)
    assert len(ids) > 1000
    assert np.all(s[ids] < e[ids]) and np.all(w[ids] > ball)
    was_parent = np.isin(ids, par0[par0 >= 0])
    assert was_parent.sum() > 50
    keep = m.culled == 0
    lmc1 = np.ascontiguousarray(_oracle_solve(oracle, N, s[keep], e[keep], w[keep], ROOT)[0])
    changed = lmc0.view(np.uint64) != lmc1.view(np.uint64)
    assert changed.sum() > 100 and np.all(lmc1 >= lmc0)
    # the same fixed point whether the culled edges are absent or present with an infinite cost
    lmc_inf = np.ascontiguousarray(_oracle_solve(oracle, N, s, e, m.dist, ROOT)[0])
    assert np.array_equal(lmc_inf.view(np.uint64), lmc1.view(np.uint64))
    assert m.cull(ball).shape[0] == 0                            # idempotent
    print(f"{len(s)} edges, {len(ids)} culled at ball {ball:.3f}, {int(was_parent.sum())} parent edges, "
          f"{int(changed.sum())} nodes change rrtLMC")


def test_a_swept_sphere_blocks_an_edge_the_cull_takes(oracle, scene):
    pts, s, e, w = scene
    sphere = DeltaScene(oracle).sphere
    mm = MirrorModel(oracle)
    mm.nodes_append(pts)
    mm.append(s, e)
    mm.spheres_set(sphere)
    blocked = mm.sweep_row(0, RR + CM.DELTA + SPHERE_RADIUS, RR)
    assert len(blocked) > 0
    m = CM.CullModel(pts, s, e)
    m.block(blocked)
    ids = m.cull(CM.ball(N, BALL_CONSTANT))
    assert np.isin(blocked, ids).any()                           # a blocked edge (+Inf > ball) is culled
    assert np.all(np.isinf(m.dist0[ids]))


def test_lattice_cases_hold_the_ball_exactly():
    # (0, 0, 0) -> (3, 4, 0) on the quarter lattice: length 5 exactly, kept at ball 5, culled just below
    pts = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.25, 0.0, 0.0], [3.0, 4.25, 0.0]])
    m = CM.CullModel(pts, [0, 1, 0, 2], [1, 0, 3, 2])
    assert m.dist[0] == 5.0 == m.dist[1]
    assert m.would_cull(5.0).tolist() == [2]                     # only the longer one
    assert m.would_cull(np.nextafter(5.0, 0.0)).tolist() == [0, 2]
    # the line: cost 1 = ball is kept in every pattern
    for ne in (1, 65, 257):
        for pattern in CM.PATTERNS:
            s, e, c = CM.line_pattern(ne, pattern)
            lm = CM.CullModel(CM.line_nodes(), s, e)
            assert np.array_equal(lm.would_cull(1.0), np.flatnonzero(c)), (ne, pattern)
            if ne > 1 and pattern != "all":
                assert (lm.dist[~c] == 1.0).any()


def test_odd_costs_and_the_renumbering():
    pts = CM.line_nodes(6)
    m = CM.CullModel(pts, [0, 0, 0, 3, 2, 1, 0], [2, 3, 4, 0, 2, 5, 5])
    m.set_dist(1, [np.nan])
    m.block([2])
    assert m.cull(1.0).tolist() == [0, 2, 5, 6]                 # NaN kept, +Inf culled, start >= end never
    assert m.cull(1.0, nodes=[0, 1, 0]).shape[0] == 0
    remap, removed = m.compact()
    assert removed == 4 and remap.tolist() == [-1, 0, -1, 1, 2, -1, -1]
    assert m.start.tolist() == [0, 3, 2] and m.end.tolist() == [3, 0, 2] and not m.culled.any()
    assert np.isnan(m.dist[0]) and m.dist[1:].tolist() == [3.0, 0.0]
    sub = CM.CullModel(pts, [0, 1, 0], [2, 4, 5])
    assert sub.cull(1.0, nodes=[1]).tolist() == [1]              # only the listed start node
