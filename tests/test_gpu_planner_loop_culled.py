"""The device-resident iteration of test_gpu_planner_loop_linked.py with cullCurrentNeighbors in it: batches of 256 samples
against the spheres of building2, ball constant 30.  Grown from the root alone the tree has 1, 11, 42, 122, 275 and 482
nodes before its first six batches, and the ball leaves delta = 8 only in the sixth (7.02): six batches from the root
cull in the last one alone, and no later batch ever runs on a compacted mirror.  So the tree is grown by PRE = 4 batches
of the same loop first, and the six batches that count start from a tree of 275 nodes, where the ball goes from 8 to
about 5 -- the cull bites from the second of them on.  One context never sees a list or an edge id on the host:
extend_select -> nodes_append -> graph_edges_append_selected -> graph_edges_cull(ball of the batch, every node) ->
graph_cost_update_delta, and graph_edges_compact after the second and the fourth of the six; both compactions remove
edges, and four batches run on a mirror that was compacted with a kept solve (append on the swapped buffers, cull, a
resumed delta with the in-edge index rebuilt).  Its twin is fed from the host: the lists fetched and linked by
tests/edges_from_lists_model.py, the cull decided by tests/cull_model.py and sent as graph_edges_set_dist(+Inf), and at
the compaction points its mirror cleared and rebuilt from the model's survivors.  Mirrors, delta reports and the final
rrtLMC must be identical; after a compaction both mirrors carry the new ids, the parent edges the twin reports after its
rebuild must be the device's through remap, and the reports of the batches that follow are compared id for id."""
import json
import os

import numpy as np
import pytest

import cull_model as CM
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context

from edges_from_lists_model import edges_from_lists, feed_reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RR = 0.5
BALL_CONSTANT = 30.0
PRE, BATCHES, B = 4, 6, 256         # batches that pre-grow the tree (same loop, same checks); the batches that count
COMPACT_AFTER = (PRE + 1, PRE + 3)  # the second and the fourth batch of the six
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _set_inf(ctx, ids):
    ids = np.asarray(ids, dtype=np.int64)
    if len(ids):
        for run in np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1):
            ctx.graph_edges_set_dist(int(run[0]), np.full(len(run), INF))


def _same_mirror(dev, host, hm, what):
    assert dev.n_graph_edges == host.n_graph_edges == hm.ne, what
    gd, gh = dev.graph_edges_get(), host.graph_edges_get()
    assert np.array_equal(gd[0], gh[0]) and np.array_equal(gd[1], gh[1]), what
    assert np.array_equal(_bits(gd[2]), _bits(gh[2])) and np.array_equal(_bits(gd[3]), _bits(gh[3])), what
    assert np.array_equal(gd[0], hm.start) and np.array_equal(_bits(gd[2]), _bits(hm.dist)), what
    assert np.array_equal(_bits(gd[3]), _bits(hm.dist0)), what
    assert np.array_equal(dev.graph_edges_culled(), hm.culled), what


def test_culled_linked_loop_matches_the_host_fed_loop():
    sph = np.asarray(json.load(open(os.path.join(HERE, "golden", "env_inputs.json")))["building2_spheres"], dtype=np.float64)
    rng = np.random.default_rng(77)
    root = np.array([[0.0, 0.0, 0.0]])
    hm = CM.CullModel(np.zeros((0, 3)), [], [], dist=[])            # the twin's mirror, column by column
    par_known = np.zeros(0, dtype=np.int32)                         # parent edge of every node as last reported
    culled_total = culled_parents = 0
    removed, culled_after_compaction = [], []       # per compaction; per batch that ran on a compacted mirror
    with Context(3) as dev, Context(3) as host:
        for c in (dev, host):
            c.spheres_set(sph)
            c.nodes_append(root)
            c.node_cost_set(0, [0.0])
        for b in range(PRE + BATCHES):
            n = host.n_nodes
            r = CM.ball(n, BALL_CONSTANT)
            Q = rng.uniform(CM.LO, CM.HI, (B, 3))
            # ---- the host-fed step
            sel_h = host.extend_select(Q, r, RR, want_lists=True)
            ins = sel_h["status"] == _capi.RRTX_SEL_OK
            node_of = np.full(B, -1, dtype=np.int32)
            node_of[ins] = n + np.arange(int(ins.sum()), dtype=np.int32)
            model = edges_from_lists(sel_h["offsets"], sel_h["idx"], sel_h["cost"], sel_h["cost"], sel_h["hit_out"],
                                     sel_h["hit_in"], node_of)
            host.nodes_append(Q[ins])
            first_h = feed_reference(host, model)
            assert first_h == hm.ne
            hm.append(model["start"], model["end"], dist=model["cost"])
            hm.block(first_h + np.flatnonzero(model["blocked"]))
            ids = hm.cull(r)
            _set_inf(host, ids)
            culled_total += len(ids)
            if removed and removed[-1] > 0:
                culled_after_compaction.append(len(ids))
            culled_parents += int(np.isin(ids, par_known[par_known >= 0]).sum())
            delta_h = host.graph_cost_update_delta(0, store=True)
            # ---- the linked step: neither a list nor an edge id leaves the device
            sel_d = dev.extend_select(Q, r, RR)
            for k in ("status", "parent_idx", "rw_offsets", "rw_node"):
                assert np.array_equal(sel_d[k], sel_h[k]), (b, k)
            assert np.array_equal(_bits(sel_d["lmc_new"]), _bits(sel_h["lmc_new"])), b
            dev.nodes_append(Q[ins])
            first_d, added, _ = dev.graph_edges_append_selected(node_of)
            assert first_d == first_h and added == len(model["start"]), b
            assert dev.graph_edges_cull(r) == len(ids), b
            delta_d = dev.graph_cost_update_delta(0, store=True)
            # ---- after every batch: the same mirror, the same report
            _same_mirror(dev, host, hm, b)
            assert np.array_equal(delta_d[0], delta_h[0]) and np.array_equal(_bits(delta_d[1]), _bits(delta_h[1])), b
            assert np.array_equal(delta_d[2], delta_h[2]), b
            par_known = np.concatenate([par_known, np.full(host.n_nodes - len(par_known), -1, dtype=np.int32)])
            par_known[delta_h[0]] = delta_h[2]
            print(f"batch {b}: tree {n}, ball {r:.3f}, {added} edges, {len(ids)} culled, delta {len(delta_h[0])} nodes")
            if b in COMPACT_AFTER:
                remap, n_removed = dev.graph_edges_compact()
                want_remap, want_removed = hm.compact()
                assert n_removed == want_removed and np.array_equal(remap, want_remap), b
                removed.append(n_removed)
                host.graph_edges_clear()                            # the twin's mirror, rebuilt from the survivors
                assert host.graph_edges_append(hm.start, hm.end) == 0
                host.graph_edges_set_dist(0, hm.dist0)
                host.graph_edges_block(np.flatnonzero(np.isinf(hm.dist) & np.isfinite(hm.dist0)).astype(np.int32))
                _same_mirror(dev, host, hm, (b, "compacted"))
                # the device carries its solve and its baseline over: nothing to report.  The twin has forgotten both
                # with its mirror and reports every node: the parent edges it names are the device's through remap.
                assert len(dev.graph_cost_update_delta(0, store=True)[0]) == 0, b
                node, lmc, par, _ = host.graph_cost_update_delta(0, store=True)
                par_known = np.where(par_known >= 0, remap[np.maximum(par_known, 0)], -1).astype(np.int32)
                assert (par_known[par_known >= 0] >= 0).all()
                full_h = np.full(host.n_nodes, -1, dtype=np.int32)
                full_h[node] = par
                assert np.array_equal(full_h, par_known), b
                lmc_d, par_d, _ = dev.graph_cost_update(0)
                assert np.array_equal(par_d, par_known) and np.array_equal(_bits(lmc_d[node]), _bits(lmc)), b
        lmc_d, par_d, _ = dev.graph_cost_update(0)
        lmc_h, par_h, _ = host.graph_cost_update(0)
        assert np.array_equal(_bits(lmc_d), _bits(lmc_h)) and np.array_equal(par_d, par_h)
        assert host.n_nodes > 100 and np.isfinite(lmc_h).all()
        # the scene exercises what it is meant to
        print(f"culled {culled_total}, {culled_parents} of them parent edges at the time; removed {removed}; culled in the "
              f"batches after a removing compaction {culled_after_compaction}")
        assert culled_parents >= 1                                  # a culled edge was a parent edge at the time
        assert len(removed) == 2 and min(removed) > 0               # both compactions removed edges
        # at least two batches appended, culled and solved on a mirror compacted with a kept solve
        assert len(culled_after_compaction) >= 2 and sum(1 for c in culled_after_compaction if c > 0) >= 2
