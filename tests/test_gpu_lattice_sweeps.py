"""The obstacle sweeps and releases on lattice scenes (tools/soak_lattice_sweeps.py): rrtx_obstacle_sweep,
rrtx_obstacle_sweep_batch, rrtx_obstacle_release_batch, rrtx_obstacle_sweep_polygon and rrtx_obstacle_sweep_polygon_batch
on mirrors whose nodes sit exactly at search ranges, whose edges are exactly tangent to inflated spheres, lie along
polygon sides and pass through vertices, and whose root lies exactly on a range.  There the `s < thr_lt || (i == 0 &&
s < thr_root)` of the four mark kernels, the thresholds the host forms and the per-bit root rule of the 64-obstacle
words decide returned ids; scenes in general position never reach them.  Every comparison is np.array_equal against the
oracle (KDTree.within_range, sweep_edges_batch, add_new_obstacle_edges, remove_obstacle_edges, the graph solve).
tests/test_lattice_sweep_scenes.py asserts, without a device, that these scenes hold the boundary cases."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "soak_lattice_sweeps", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "soak_lattice_sweeps.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

SEED_S, SEED_P, SEED_D = 7, 7, 5                   # the seeds test_lattice_sweep_scenes.py judges


@pytest.fixture(scope="module")
def sphere_scene(oracle):
    return T.sphere_scene(SEED_S)


def test_sphere_sweeps_and_release_on_the_lattice(sphere_scene):
    """S: the burst over all 70 positions shuffled (cap = 16, then the exact total) against the oracle and the single
    call; every range one ulp up and one ulp down; edges_check_idx against ten single spheres; the release of 66
    entries (64 + 2) after the sweeps of positions 0 .. 39 were blocked."""
    s = sphere_scene
    o = T.check_spheres(s, solve=False)
    assert o["rows"] == 3 * 70 + 66 and o["ids"] > 60_000


def test_sphere_block_and_unblock_in_the_call_on_the_lattice(sphere_scene):
    """S: block=True on the sweeps of positions 0 .. 39 against graph_edges_block(union) on a second context, then
    unblock=True on the release of the leaving set against graph_edges_unblock(union), through graph_cost_update: equal
    rrtLMC from both contexts, equal to the oracle's solve, parent edges where a single edge attains the minimum."""
    o = T.check_spheres_marks(sphere_scene)
    assert o["blocked"] > 100 and 0 < o["freed"] < o["blocked"]
    assert o["lmc_changed_by_block"] > 0 and o["lmc_changed_by_unblock"] > 0


def test_polygon_sweeps_on_the_lattice(oracle):
    """P: the burst over all 70 positions (64 + 6) against add_new_obstacle_edges and the single call, mode 1 against
    remove_obstacle_edges after the union of the first 20 rows is blocked; both again with DELTA + 2^-30; the root's
    row at DELTA - 2^-30."""
    s = T.polygon_scene(SEED_P)
    o = T.check_polygons(s)
    assert o["rows"] == 2 * 70 + 2 * 10 and o["ids"] > 50_000


@pytest.mark.parametrize("root_planted", [False, True])
def test_dubins_sweeps_on_the_lattice(oracle, root_planted):
    """D: the burst (70 entries, two groups) and the single call against add_new_obstacle_edges(dubins=True), with
    nodes planted exactly on the ranges of the polygons centred at the origin, one of them the root in the second
    variant; both again with DELTA + 2^-30; once with RRTX_OPT_ROOT_RULE = 0 against the single calls."""
    s = T.dubins_scene(SEED_D, root_planted=root_planted)
    o = T.check_dubins(s)
    assert o["rows"] == 2 * 70 and o["ids"] > 5000
    assert (o["no_root_rule_lost"] > 0) == root_planted        # the planted root's out-edges are what the rule adds
