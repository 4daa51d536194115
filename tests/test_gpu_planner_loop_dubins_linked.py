"""The device-resident Dubins iteration end to end, the twin of tests/test_gpu_planner_loop_linked.py: batches of
samples from the root alone in the scene of tests/test_gpu_planner_loop_dubins_batched.py (its six shrunk polygons,
R = 4, RMIN = 0.5, RR = 0.25, samples in [-10, 10]^2 with free theta, theta wrapped).  One context never sees a neighbour
list on the host: extend_select_dubins -> nodes_append of the samples with status OK -> graph_edges_append_selected ->
graph_cost_update_delta (store = 1, which leaves rrtLMC where the next extend_select_dubins reads it).  A second context
runs the host-fed step: the lists fetched, tests/edges_from_lists_model.py applied on the host with the two cost arrays,
and the edges sent up with graph_edges_append + graph_edges_set_dist + graph_edges_block.  After every batch the two
mirrors and the two delta reports must be identical, and at the end rrtLMC and the parent edge of every node.

Eight batches of 128 samples, chosen so that the host-fed loop alone meets the three conditions asserted at the end
(conditions on the scene, not measurements of the code under test).  Seen there: the tree grows 1 -> 12 -> 42 -> 94 ->
175 -> 282 -> 394 -> 515 -> 641 nodes; 1 165 blocked out-edges are linked (the first two in batch 1); every batch from
the third on lowers earlier nodes (8, 25, 106, 107, 133, 297 of them)."""
import numpy as np
import pytest

from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

from edges_from_lists_model import edges_from_lists, feed_reference
from test_gpu_planner_loop_dubins_batched import R, RMIN, ROOT, RR, TWO_PI, _polygons

pytestmark = pytest.mark.gpu
BATCHES, B, SEED = 8, 128, 31


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_linked_dubins_loop_matches_the_host_fed_loop():
    rng = np.random.default_rng(SEED)
    blocked_out = rewired = 0
    with Context(4) as dev, Context(4) as host:
        for c in (dev, host):
            c.set_wrap(3, TWO_PI)
            c.polygons_set(_polygons())
            c.nodes_append(ROOT[None])
            c.node_cost_set(0, [0.0])
        for b in range(BATCHES):
            n = host.n_nodes
            Q = np.column_stack([rng.uniform(-10.0, 10.0, (B, 2)), np.zeros(B), rng.uniform(0.0, TWO_PI, B)])
            # ---- the host-fed step
            sel_h = host.extend_select_dubins(Q, R, RR, RMIN, want_lists=True)
            ins = sel_h["status"] == _capi.RRTX_SEL_OK
            node_of = np.full(B, -1, dtype=np.int32)
            node_of[ins] = n + np.arange(int(ins.sum()), dtype=np.int32)
            model = edges_from_lists(sel_h["offsets"], sel_h["idx"], sel_h["cost_out"], sel_h["cost_in"], sel_h["hit_out"],
                                     sel_h["hit_in"], node_of)
            host.nodes_append(Q[ins])
            first_h = feed_reference(host, model)
            delta_h = host.graph_cost_update_delta(0, store=True)
            # ---- the linked step: no list leaves the device
            sel_d = dev.extend_select_dubins(Q, R, RR, RMIN)
            for k in ("status", "parent_idx", "rw_offsets", "rw_node", "nearest_idx"):
                assert np.array_equal(sel_d[k], sel_h[k]), (b, k)
            assert np.array_equal(_bits(sel_d["lmc_new"]), _bits(sel_h["lmc_new"])), b
            dev.nodes_append(Q[ins])
            first_d, added, row_first = dev.graph_edges_append_selected(node_of)
            delta_d = dev.graph_cost_update_delta(0, store=True)
            # ---- after every batch: the same mirror, the same report
            assert first_d == first_h and added == len(model["start"]) and np.array_equal(row_first, model["row_first"]), b
            assert dev.n_graph_edges == host.n_graph_edges == first_h + added, b
            gd, gh = dev.graph_edges_get(), host.graph_edges_get()
            assert np.array_equal(gd[0], gh[0]) and np.array_equal(gd[1], gh[1]), b
            assert np.array_equal(_bits(gd[2]), _bits(gh[2])) and np.array_equal(_bits(gd[3]), _bits(gh[3])), b
            assert np.array_equal(delta_d[0], delta_h[0]) and np.array_equal(_bits(delta_d[1]), _bits(delta_h[1])), b
            assert np.array_equal(delta_d[2], delta_h[2]), b
            blocked_out += int(model["blocked"].sum())
            rewired += int((delta_h[0] < n).sum()) if b else 0
            print(f"batch {b}: tree {n}, {int(ins.sum())} inserted, {added} edges, {int(model['blocked'].sum())} blocked "
                  f"out-edges, delta {len(delta_h[0])} nodes ({int((delta_h[0] < n).sum())} earlier ones)")
        lmc_d, par_d, _ = dev.graph_cost_update(0)
        lmc_h, par_h, _ = host.graph_cost_update(0)
        assert np.array_equal(_bits(lmc_d), _bits(lmc_h)) and np.array_equal(par_d, par_h)
        # the scene does its work: the tree grows, blocked out-edges were linked, and a batch lowered earlier nodes
        assert host.n_nodes > 100 and np.isfinite(lmc_h).all()
        assert blocked_out >= 1 and rewired >= 1
