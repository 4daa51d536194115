"""A Dubins planner loop with the extend side batched, driven through drrt: after 400 iterations one sample per call
(drrt.extend_candidates_dubins on a batch of one), the remaining samples go through in batches of 32 -- one
drrt.extend_candidates_dubins call (the lists against the tree as it stood, in the wrapped space) and one
drrt.extend_candidates_self_dubins call (the lists of the batch's samples among themselves) per batch.  The host then
runs findBestParent over cost_out / hit_out, insertion and the one-hop rewire over cost_in / hit_in sample by sample
over the merged lists: the tree list, then the batch list with every earlier sample mapped to the node index it received
(samples that were not inserted are dropped), and appends the batch's nodes in one call.  Positions, parents and the
rrtLMC bit patterns must equal the tree a CPU loop grows one sample at a time from the oracle alone."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import drrt, synth

pytestmark = pytest.mark.gpu
N_ITER, N_SEQ, BATCH, SEED = 1000, 400, 32, 11
R, RMIN, RR = 4.0, 0.5, 0.25
TWO_PI = 2.0 * math.pi
ROOT = np.array([0.0, 0.0, 0.0, 1.0])


def _polygons():
    out = []
    for p in synth.polygons(6, seed=12):
        p = p * (10.0 / synth.WORLD)
        c = p.mean(axis=0)
        out.append(c + (p - c) * 0.35)
    return out


def _samples():
    rng = np.random.default_rng(SEED)
    return [np.array([*rng.uniform(-10.0, 10.0, 2), 0.0, rng.uniform(0.0, TWO_PI)]) for _ in range(N_ITER)]


def _adopt(idx, cost_out, cost_in, hit_out, hit_in, lmc, parent, new):
    """findBestParent over the out edges and, with a parent, the one-hop rewire over the in edges of one sample's list
    (ascending node index); returns (parent, lmc)"""
    best, best_parent = math.inf, -1
    for j, c, blocked in zip(idx, cost_out, hit_out):
        if not blocked and best > lmc[j] + c:
            best, best_parent = lmc[j] + c, int(j)
    if best_parent < 0:
        return -1, math.inf
    for j, c, blocked in zip(idx, cost_in, hit_in):
        if blocked or j == 0:
            continue
        if lmc[j] > best + c and best_parent != j:
            parent[j] = new
            lmc[j] = best + c
    return best_parent, best


def _grow_cpu(oracle, samples):
    """one sample at a time, from the oracle alone; also the length of every sample's list and the number of list
    entries of the batched phase that are nodes of the sample's own batch"""
    ps = oracle.PolygonSet(_polygons())
    tree = oracle.KDTree(4, [3], [TWO_PI])
    pos, parent, lmc = [ROOT], [-1], [0.0]
    tree.insert(ROOT)
    lens, own_batch = [], 0
    batch_first = {}                                   # batch number -> tree size when the batch began
    for it, p in enumerate(samples):
        if it >= N_SEQ:
            batch_first.setdefault((it - N_SEQ) // BATCH, len(pos))
        if oracle.point_check_polygons(ps, p, RR)[0]:
            continue
        idx, _ = tree.within_range(R, p)
        idx = np.sort(idx)
        lens.append((it, len(idx)))
        if len(idx) == 0:                              # the closestNode rule (R/DRRT_Q.jl:1930-1935)
            idx = np.array([tree.nearest(p)[0]], dtype=np.int32)
        elif it >= N_SEQ:
            own_batch += int((idx >= batch_first[(it - N_SEQ) // BATCH]).sum())
        nodes = np.array(pos)
        c = oracle.dubins_candidates_batch(p[None], np.array([0, len(idx)]), idx, nodes, RMIN, ps, RR)
        n = len(pos)
        parent.append(-1); lmc.append(math.inf)        # (slot n, dropped again without a parent)
        bp, best = _adopt(idx, c["cost_out"], c["cost_in"], c["hit_out"], c["hit_in"], lmc, parent, n)
        if bp < 0:
            parent.pop(); lmc.pop()
            continue
        assert tree.insert(p) == n
        pos.append(p); parent[n] = bp; lmc[n] = best
    return (np.array(pos), np.array(parent), np.array(lmc)), lens, own_batch


def _grow_gpu(samples):
    tree = drrt.HipTree(4, wraps=[4], wrapPoints=[TWO_PI])
    S = drrt.CSpace(4, -1.0, [-10.0, -10.0, 0.0, 0.0], [10.0, 10.0, 0.0, TWO_PI], ROOT, ROOT)
    S.robotRadius, S.minTurningRadius = RR, RMIN
    for poly in _polygons():
        drrt.addObsToCSpace(S, drrt.Obstacle(3, poly))
    pos, parent, lmc = [ROOT], [-1], [0.0]
    drrt.kdInsert(tree, drrt.RRTNode(ROOT))
    for p in samples[:N_SEQ]:                          # one sample per call
        cand = drrt.extend_candidates_dubins(tree, S, p[None], R)
        if cand["sample_unsafe"][0]:
            continue
        idx = cand["idx"]
        assert (np.diff(idx) > 0).all()
        cols = [cand[k] for k in ("cost_out", "cost_in", "hit_out", "hit_in")]
        if len(idx) == 0:                              # the closestNode rule: one edge each way
            near = int(cand["nearest_idx"][0])
            q = pos[near]
            co, _, ho, _ = tree.ctx.dubins_edges_check(p[None], q[None], RMIN, RR)
            ci, _, hi, _ = tree.ctx.dubins_edges_check(q[None], p[None], RMIN, RR)
            idx, cols = np.array([near]), [co, ci, ho, hi]
        n = len(pos)
        parent.append(-1); lmc.append(math.inf)
        bp, best = _adopt(idx, *cols, lmc, parent, n)
        if bp < 0:
            parent.pop(); lmc.pop()
            continue
        node = drrt.RRTNode(p)
        drrt.kdInsert(tree, node)
        assert node.index == n
        pos.append(p); parent[n] = bp; lmc[n] = best
    self_used = 0
    for b0 in range(N_SEQ, len(samples), BATCH):
        batch = np.array(samples[b0:b0 + BATCH])
        n0 = len(pos)
        cand = drrt.extend_candidates_dubins(tree, S, batch, R)
        self_ = drrt.extend_candidates_self_dubins(tree, S, batch, R, skip=cand["sample_unsafe"])
        node_of = np.full(len(batch), -1, dtype=np.int64)
        inserted = []
        for j, p in enumerate(batch):
            if cand["sample_unsafe"][j]:
                assert self_["offsets"][j] == self_["offsets"][j + 1]
                continue
            a0, a1 = cand["offsets"][j], cand["offsets"][j + 1]
            s0, s1 = self_["offsets"][j], self_["offsets"][j + 1]
            mapped = node_of[self_["idx"][s0:s1]]
            keep = mapped >= 0
            self_used += int(keep.sum())
            idx = np.concatenate([cand["idx"][a0:a1], mapped[keep]])
            assert (np.diff(idx) > 0).all()            # ascending node index, as the reference's list
            assert len(idx) > 0                        # (the closestNode rule is not part of the batched phase)
            cols = [np.concatenate([cand[k][a0:a1], self_[k][s0:s1][keep]])
                    for k in ("cost_out", "cost_in", "hit_out", "hit_in")]
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
    return (np.array(pos), np.array(parent), np.array(lmc)), self_used


def test_batched_dubins_extend_grows_the_cpu_tree(oracle):
    samples = _samples()
    c, lens, own_batch = _grow_cpu(oracle, samples)
    # no sample of the batched phase has an empty ball on the oracle's side (the closestNode rule would need a nearest
    # search over the batch), and the batched phase does meet nodes of a sample's own batch
    assert all(n > 0 for it, n in lens if it >= N_SEQ)
    assert own_batch > 0
    g, self_used = _grow_gpu(samples)
    print(f"{len(c[0])} nodes on the CPU, {len(g[0])} on the device; {own_batch} / {self_used} list entries from a sample's "
          f"own batch")
    assert len(g[0]) == len(c[0]) and len(g[0]) > 0.7 * N_ITER
    assert self_used > 0 and self_used == own_batch
    assert np.array_equal(g[0], c[0])
    assert np.array_equal(g[1], c[1])
    assert np.array_equal(g[2].view(np.uint64), c[2].view(np.uint64))            # bit-exact costs-to-goal
