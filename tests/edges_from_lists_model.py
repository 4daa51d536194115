"""numpy restatement of "the extend lists become mirror edges" (include/rrtx.h): what
rrtx_graph_edges_append_lists[_dev] / rrtx_graph_edges_append_selected append, as the arrays the existing sequence
rrtx_graph_edges_append + rrtx_graph_edges_set_dist + rrtx_graph_edges_block takes.

For j = 0 .. nq-1 with v = node_of[j] >= 0, in that order, and for every surviving entry e of row j in list order
(u = idx[e], or node_of[idx[e]] with idx_is_batch; an entry whose mapped value is negative is dropped):
  1. the out-edge v -> u, always: original cost cost_out[e], blocked when hit_out[e] != 0;
  2. the in-edge u -> v, only when hit_in[e] == 0: cost cost_in[e], never blocked.
"""
import numpy as np


def edges_from_lists(offsets, idx, cost_out, cost_in, hit_out, hit_in, node_of, idx_is_batch=False):
    """Returns a dict: start, end (int32), cost (float64, the original cost), blocked (bool), row_first (int64,
    nq + 1: the CSR of every sample's edges, an empty row for a sample that was not inserted) and dropped (the entries
    of inserted samples that did not survive the mapping)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    node_of = np.asarray(node_of, dtype=np.int32)
    nq = node_of.shape[0]
    assert offsets.shape[0] == nq + 1
    start, end, cost, blocked = [], [], [], []
    row_first = np.zeros(nq + 1, dtype=np.int64)
    dropped = 0
    for j in range(nq):
        row_first[j] = len(start)
        v = int(node_of[j])
        if v < 0:
            continue
        for e in range(int(offsets[j]), int(offsets[j + 1])):
            u = int(idx[e])
            if idx_is_batch:
                assert 0 <= u < nq
                u = int(node_of[u])
                if u < 0:
                    dropped += 1
                    continue
            start.append(v); end.append(u); cost.append(float(cost_out[e])); blocked.append(hit_out[e] != 0)
            if hit_in[e] == 0:
                start.append(u); end.append(v); cost.append(float(cost_in[e])); blocked.append(False)
    row_first[nq] = len(start)
    return dict(start=np.asarray(start, dtype=np.int32), end=np.asarray(end, dtype=np.int32),
                cost=np.asarray(cost, dtype=np.float64), blocked=np.asarray(blocked, dtype=bool), row_first=row_first,
                dropped=dropped)


def feed_reference(ctx, model):
    """The existing sequence on a context: append, set_dist with the original costs, block of the blocked out-edges.
    Returns the id of the first edge."""
    first = ctx.n_graph_edges
    if model["start"].shape[0] == 0:
        return first
    first = ctx.graph_edges_append(model["start"], model["end"])
    ctx.graph_edges_set_dist(first, model["cost"])
    ids = first + np.nonzero(model["blocked"])[0]
    if ids.shape[0]:
        ctx.graph_edges_block(ids.astype(np.int32))
    return first
