"""The device-resident iteration end to end: six batches of 256 samples from the root alone, against the spheres of the
reference's environments/building2.txt (two of the samples are planted, see below).  One context never sees a neighbour list on the host:
extend_select -> nodes_append of the samples with status OK -> graph_edges_append_selected -> graph_cost_update_delta
(store = 1, which leaves rrtLMC where the next extend_select reads it).  A second context runs the same loop the way it
had to be run before: the lists fetched, tests/edges_from_lists_model.py applied on the host, and the edges sent up
with graph_edges_append + graph_edges_set_dist + graph_edges_block.  After every batch the two mirrors and the two delta
reports must be identical, and at the end rrtLMC of every node bit for bit."""
import json
import math
import os

import numpy as np
import pytest

from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

from edges_from_lists_model import edges_from_lists, feed_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
RR = 0.5                    # R/experimentsForRRTQX.jl:38
DELTA, BALL_CONSTANT = 8.0, 80.0
LO, HI = -20.0, 20.0
BATCHES, B = 6, 256


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_linked_loop_matches_the_host_fed_loop():
    sph = np.asarray(json.load(open(os.path.join(ROOT, "golden", "env_inputs.json")))["building2_spheres"], dtype=np.float64)
    rng = np.random.default_rng(77)
    root = np.array([[0.0, 0.0, 0.0]])             # the middle of the building: blocked edges from early on
    # Two samples a unit apart, the first in batch 0, the second in batch 1, beside the sphere nearest the root: both are
    # clear of it (4.011 from its centre against 4.0) and see the root, the middle of the edge between them is not
    # (3.98).  Only so short an edge between two safe points is blocked: the reference's distancePointToSegment divides
    # the dot product by the edge's length, not its square, and tests a longer edge next to one of its ends.
    c, reach = sph[14, :3], sph[14, 3] + RR
    u = -c / np.linalg.norm(c)
    w = np.cross(u, [0.0, 0.0, 1.0])
    w /= np.linalg.norm(w)
    planted = [c + (reach - 0.02) * u + 0.5 * w, c + (reach - 0.02) * u - 0.5 * w]
    blocked_out = rewired = 0
    with Context(3) as dev, Context(3) as host:
        for c in (dev, host):
            c.spheres_set(sph)
            c.nodes_append(root)
            c.node_cost_set(0, [0.0])
        for b in range(BATCHES):
            n = host.n_nodes
            r = min(DELTA, BALL_CONSTANT * (math.log(1 + n) / n) ** (1.0 / 3.0))
            Q = rng.uniform(LO, HI, (B, 3))
            if b < 2:
                Q[0] = planted[b]
            # ---- the host-fed step
            sel_h = host.extend_select(Q, r, RR, want_lists=True)
            ins = sel_h["status"] == _capi.RRTX_SEL_OK
            node_of = np.full(B, -1, dtype=np.int32)
            node_of[ins] = n + np.arange(int(ins.sum()), dtype=np.int32)
            model = edges_from_lists(sel_h["offsets"], sel_h["idx"], sel_h["cost"], sel_h["cost"], sel_h["hit_out"],
                                     sel_h["hit_in"], node_of)
            host.nodes_append(Q[ins])
            first_h = feed_reference(host, model)
            delta_h = host.graph_cost_update_delta(0, store=True)
            # ---- the linked step: no list leaves the device
            sel_d = dev.extend_select(Q, r, RR)
            for k in ("status", "parent_idx", "rw_offsets", "rw_node"):
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
            print(f"batch {b}: tree {n}, r {r:.3f}, {int(ins.sum())} inserted, {added} edges, {int(model['blocked'].sum())} blocked "
                  f"out-edges, delta {len(delta_h[0])} nodes ({int((delta_h[0] < n).sum())} earlier ones)")
        lmc_d, par_d, _ = dev.graph_cost_update(0)
        lmc_h, par_h, _ = host.graph_cost_update(0)
        assert np.array_equal(_bits(lmc_d), _bits(lmc_h)) and np.array_equal(par_d, par_h)
        assert host.n_nodes > 100 and np.isfinite(lmc_h).all()
        # the scene exercises what it is meant to: blocked out-edges were linked, and a batch lowered earlier nodes
        assert blocked_out >= 1 and rewired >= 1
