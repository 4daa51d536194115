"""A Dubins planner loop grown from the root alone in batches of 32, driven through drrt: per batch one
drrt.extend_candidates_dubins call (the lists against the tree as it stood, in the wrapped space), one
drrt.extend_candidates_self_dubins call (the lists of the batch's samples among themselves) and one
drrt.extend_closest_self_dubins call for the samples whose tree list is empty.  A sample whose merged list is empty is
linked by the closestNode rule (R/DRRT_Q.jl:1930-1935): the first inserted entry of its row if its key is below the
distance of the tree's nearest node, else that node; a row of k with no inserted entry and its k-th key below that
distance is exhausted and the host searches the batch itself.  Positions, parents and the rrtLMC bit patterns must equal
the tree a CPU loop grows one sample at a time from the oracle alone.  How often the rule ran, with an own-batch closest
node, through a ghost, at which rank, and which rows a list of k exhausts is derived from the CPU run."""
import math

import numpy as np
import pytest

import extend_closest_dubins_model as M
from rrtqx_3d_amd import drrt, synth
from test_gpu_planner_loop_dubins_batched import _adopt

pytestmark = pytest.mark.gpu
BATCH, SEED = 32, 11
RMIN, RR = 0.5, 0.25
TWO_PI = 2.0 * math.pi
THETA = ((3,), (TWO_PI,))
ROOT = np.array([0.0, 0.0, 0.0, 1.0])
# name: polygons, the factor they are shrunk by about their mean, ball radius, samples
SCENES = {"open": (6, 0.35, 4.0, 1000), "dense": (24, 0.6, 1.5, 600)}


def _polygons(name):
    m, shrink, _, _ = SCENES[name]
    out = []
    for p in synth.polygons(m, seed=12):
        p = p * (10.0 / synth.WORLD)
        c = p.mean(axis=0)
        out.append(c + (p - c) * shrink)
    return out


def _samples(name):
    rng = np.random.default_rng(SEED)
    return [np.array([*rng.uniform(-10.0, 10.0, 2), 0.0, rng.uniform(0.0, TWO_PI)]) for _ in range(SCENES[name][3])]


def _grow_cpu(oracle, name):
    """one sample at a time, from the oracle alone; the log has per iteration the sample, whether it is unsafe, the
    length of its list, the closest node where the list is empty, the node it became (-1: none) and the size of the tree
    when its batch began"""
    ps = oracle.PolygonSet(_polygons(name))
    r = SCENES[name][2]
    tree = oracle.KDTree(4, [3], [TWO_PI])
    pos, parent, lmc = [ROOT], [-1], [0.0]
    tree.insert(ROOT)
    log = []
    for it, p in enumerate(_samples(name)):
        size = len(pos) if it % BATCH == 0 else log[-1]["size"]
        e = dict(p=p, unsafe=bool(oracle.point_check_polygons(ps, p, RR)[0]), n_list=-1, near=-1, node=-1, size=size)
        log.append(e)
        if e["unsafe"]:
            continue
        idx, _ = tree.within_range(r, p)
        idx = np.sort(idx)
        e["n_list"] = len(idx)
        if len(idx) == 0:                              # the closestNode rule
            e["near"] = int(tree.nearest(p)[0])
            idx = np.array([e["near"]], dtype=np.int32)
        c = oracle.dubins_candidates_batch(p[None], np.array([0, len(idx)]), idx, np.array(pos), RMIN, ps, RR)
        n = len(pos)
        parent.append(-1); lmc.append(math.inf)        # (slot n, dropped again without a parent)
        bp, best = _adopt(idx, c["cost_out"], c["cost_in"], c["hit_out"], c["hit_in"], lmc, parent, n)
        if bp < 0:
            parent.pop(); lmc.pop()
            continue
        assert tree.insert(p) == n
        pos.append(p); parent[n] = bp; lmc[n] = best
        e["node"] = n
    return (np.array(pos), np.array(parent), np.array(lmc)), log


def _wrapped_s(p, nodes):
    """min over the copies of p of sq4(copy, node), per node"""
    return M.s_all(np.vstack([nodes, p[None]]), THETA)[0][-1, :-1]


def _rule_figures(log, pos, k):
    """From the CPU run, per batch: the samples with an empty ball, those whose closest node is a sample of their own
    batch, how many of those are closest through the theta ghost, the rank of that sample among the live earlier ones by
    (s, i), the safe samples that were not inserted, and the iterations whose row a list of k exhausts: a live sample
    with an empty ball, at least k live earlier samples, none of the first k inserted, and the k-th nearer than the
    nearest node of the tree as it stood when the batch began."""
    fig = dict(empty=0, own_batch=0, via_ghost=0, ranks=[], safe_not_inserted=0, exhausted=[])
    for b0 in range(0, len(log), BATCH):
        rows = log[b0:b0 + BATCH]
        first = rows[0]["size"]
        Q = np.array([e["p"] for e in rows])
        ranked = M.ranked_rows(Q, THETA, skip=[e["unsafe"] for e in rows])
        sample_of = {e["node"]: j for j, e in enumerate(rows) if e["node"] >= 0}
        for j, e in enumerate(rows):
            if e["unsafe"]:
                continue
            fig["safe_not_inserted"] += e["node"] < 0
            if e["n_list"] != 0:
                continue
            fig["empty"] += 1
            order = list(ranked[j][0])
            if len(order) >= k and not any(rows[i]["node"] >= 0 for i in order[:k]):
                to_tree = np.sqrt(_wrapped_s(e["p"], pos[:first]).min())
                if np.sqrt(ranked[j][1][k - 1]) < to_tree:
                    fig["exhausted"].append(b0 + j)
            if e["near"] >= first:
                fig["own_batch"] += 1
                rank = order.index(sample_of[e["near"]])
                fig["ranks"].append(rank)
                fig["via_ghost"] += int(ranked[j][2][rank] != 0)
    return fig


def _grow_batched(name, k):
    """every sample in batches from the root alone; returns the tree, the iterations whose row was exhausted and the
    number of times the rule ran"""
    r = SCENES[name][2]
    tree = drrt.HipTree(4, wraps=[4], wrapPoints=[TWO_PI])
    S = drrt.CSpace(4, -1.0, [-10.0, -10.0, 0.0, 0.0], [10.0, 10.0, 0.0, TWO_PI], ROOT, ROOT)
    S.robotRadius, S.minTurningRadius = RR, RMIN
    for poly in _polygons(name):
        drrt.addObsToCSpace(S, drrt.Obstacle(3, poly))
    pos, parent, lmc = [ROOT], [-1], [0.0]
    drrt.kdInsert(tree, drrt.RRTNode(ROOT))
    samples = _samples(name)
    exhausted, used_rule = [], 0
    fields = ("cost_out", "cost_in", "hit_out", "hit_in")
    for b0 in range(0, len(samples), BATCH):
        batch = np.array(samples[b0:b0 + BATCH])
        n0 = len(pos)
        cand = drrt.extend_candidates_dubins(tree, S, batch, r)
        unsafe = cand["sample_unsafe"]
        self_ = drrt.extend_candidates_self_dubins(tree, S, batch, r, skip=unsafe)
        want = ((np.diff(cand["offsets"]) == 0) & (unsafe == 0)).astype(np.uint8)
        clo = drrt.extend_closest_self_dubins(tree, S, batch, k, skip=unsafe, want=want, treeNearest=cand["nearest_idx"])
        node_of = np.full(len(batch), -1, dtype=np.int64)
        inserted = []
        for j, p in enumerate(batch):
            if unsafe[j]:
                continue
            a0, a1 = cand["offsets"][j], cand["offsets"][j + 1]
            s0, s1 = self_["offsets"][j], self_["offsets"][j + 1]
            mapped = node_of[self_["idx"][s0:s1]]
            keep = mapped >= 0
            idx = np.concatenate([cand["idx"][a0:a1], mapped[keep]])
            assert (np.diff(idx) > 0).all()           # ascending node index, as the reference's list
            cols = [np.concatenate([cand[f][a0:a1], self_[f][s0:s1][keep]]) for f in fields]
            if len(idx) == 0:                          # the closestNode rule
                assert want[j]
                used_rule += 1
                near_dist = cand["nearest_dist"][j]
                link = (cand["nearest_idx"][j],) + tuple(clo["tree_" + f][j] for f in fields)
                row = clo["idx"][j, :clo["count"][j]]
                ins = np.flatnonzero(node_of[row] >= 0)
                if len(ins):                           # the first entry whose sample was inserted
                    s = ins[0]
                    if clo["key"][j, s] < near_dist:
                        link = (node_of[row[s]],) + tuple(clo[f][j, s] for f in fields)
                elif clo["count"][j] == k and clo["key"][j, k - 1] < near_dist:
                    # exhausted: none of the k was inserted and a later entry may still beat the tree node; brute force
                    # over the batch, two edge checks
                    exhausted.append(b0 + j)
                    earlier = np.flatnonzero(node_of[:j] >= 0)
                    if len(earlier):
                        s_all = _wrapped_s(p, batch[earlier])
                        o = np.lexsort((earlier, s_all))[0]
                        if np.sqrt(s_all[o]) < near_dist:
                            q = batch[earlier[o]]
                            co, _, ho, _ = tree.ctx.dubins_edges_check(p[None], q[None], RMIN, RR)
                            ci, _, hi, _ = tree.ctx.dubins_edges_check(q[None], p[None], RMIN, RR)
                            link = (node_of[earlier[o]], co[0], ci[0], ho[0], hi[0])
                idx, cols = np.array([link[0]]), [np.array([v]) for v in link[1:]]
            n = len(pos)
            parent.append(-1); lmc.append(math.inf)
            bp, best = _adopt(idx, *cols, lmc, parent, n)
            if bp < 0:
                parent.pop(); lmc.pop()
                continue
            node_of[j] = n
            pos.append(p); parent[n] = bp; lmc[n] = best
            inserted.append(drrt.RRTNode(p))
        drrt.kdInsertMany(tree, inserted)              # the batch's nodes in one rrtx_nodes_append
        assert tree.treeSize == len(pos) and [n.index for n in inserted] == list(range(n0, len(pos)))
    return (np.array(pos), np.array(parent), np.array(lmc)), exhausted, used_rule


@pytest.fixture(scope="module")
def cpu_runs(oracle):
    return {name: _grow_cpu(oracle, name) for name in SCENES}


@pytest.mark.parametrize("name,k", [("open", 8), ("dense", 8), ("dense", 4)])
def test_dubins_from_the_root_alone(cpu_runs, name, k):
    c, log = cpu_runs[name]
    assert len(log) == SCENES[name][3]
    fig = _rule_figures(log, c[0], k)
    hist = {r: fig["ranks"].count(r) for r in sorted(set(fig["ranks"]))}
    print(f"{name}, k = {k}: {len(c[0])} nodes, {fig['empty']} empty balls, {fig['own_batch']} closest nodes in the own "
          f"batch ({fig['via_ghost']} through the ghost), ranks {hist}, {fig['safe_not_inserted']} safe samples not "
          f"inserted, {len(fig['exhausted'])} exhausted rows")
    assert fig["empty"] >= 20 and fig["own_batch"] >= 5 and fig["via_ghost"] >= 1
    assert max(fig["ranks"]) > 0 and fig["safe_not_inserted"] > 0
    if name == "dense":
        if k == 8:
            assert len(fig["exhausted"]) == 0
        else:
            assert len(fig["exhausted"]) >= 1
    g, exhausted, used_rule = _grow_batched(name, k)
    # the exit serves exactly the rows the list cannot: none is swallowed, none is invented
    assert used_rule == fig["empty"] and exhausted == fig["exhausted"]
    assert len(g[0]) == len(c[0])
    assert np.array_equal(g[0], c[0])
    assert np.array_equal(g[1], c[1])
    assert np.array_equal(g[2].view(np.uint64), c[2].view(np.uint64))            # bit-exact costs-to-goal
