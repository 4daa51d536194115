"""The planner loop of tests/test_gpu_planner_loop.py with the extend side batched: after 400 iterations one sample per
call, the remaining samples go through in batches of 64 -- one drrt.extend_candidates call (the lists against the tree
as it stood) and one drrt.extend_candidates_self call (the lists of the batch's samples among themselves) per batch.
The host then runs findBestParent, insertion and the one-hop rewire sample by sample over the merged lists: the tree
list, then the batch list with every earlier sample mapped to the node index it received (samples that were not
inserted are dropped), and appends the batch's nodes in one call.  The tree must equal, bit for bit, the one the CPU
oracle grows one sample at a time."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import drrt
from test_gpu_planner_loop import BALL_CONSTANT, DELTA, HI, LO, _CpuBackend, _GpuBackend, _grow, _spheres

pytestmark = pytest.mark.gpu
N_ITER, N_SEQ, BATCH, SEED = 1200, 400, 64, 7


class _RecordingCpu(_CpuBackend):
    """_CpuBackend that notes, per iteration (nearest() opens one), the length of the list candidates() returned"""

    def __init__(self, oracle, sph):
        super().__init__(oracle, sph)
        self.it, self.lens = 0, []

    def nearest(self, pos):
        self.it += 1
        return super().nearest(pos)

    def candidates(self, pos, r):
        out = super().candidates(pos, r)
        self.lens.append((self.it, len(out[0])))
        return out


def _ball(n):
    return min(DELTA, BALL_CONSTANT * ((math.log(1 + n) / n) ** (1.0 / 3)))   # R/rrtqx.jl:382


def _adopt(idx, cost, hit_out, hit_in, lmc, parent, new):
    """findBestParent and, with a parent, the one-hop rewire of _grow over one sample's list; returns (parent, lmc)"""
    best, best_parent = math.inf, -1
    for j, c, blocked in zip(idx, cost, hit_out):
        if not blocked and best > lmc[j] + c:
            best, best_parent = lmc[j] + c, int(j)
    if best_parent < 0:
        return -1, math.inf
    for j, c, blocked in zip(idx, cost, hit_in):
        if blocked or j == 0:
            continue
        if lmc[j] > best + c and best_parent != j:
            parent[j] = new
            lmc[j] = best + c
    return best_parent, best


def _grow_batched(be, samples):
    pos = [np.array([15.0, 15.0, 15.0])]
    parent, lmc = [-1], [0.0]
    be.insert(pos[0])
    for p in samples[:N_SEQ]:                       # one sample per call, as _grow
        near, _ = be.nearest(p)
        if be.unsafe(p):
            continue
        n = len(pos)
        idx, cost, hit_out, hit_in = be.candidates(p, _ball(n))
        if len(idx) == 0:
            idx = np.array([near])
            cost = np.array([be.dist(p, pos[near])])
            hit_out = np.array([be.edge_blocked(p, pos[near])])
            hit_in = np.array([be.edge_blocked(pos[near], p)])
        parent.append(-1); lmc.append(math.inf)      # (slot n, dropped again without a parent)
        bp, best = _adopt(idx, cost, hit_out, hit_in, lmc, parent, n)
        if bp < 0:
            parent.pop(); lmc.pop()
            continue
        assert be.insert(p) == n
        pos.append(p); parent[n] = bp; lmc[n] = best
    for b0 in range(N_SEQ, len(samples), BATCH):
        batch = np.array(samples[b0:b0 + BATCH])
        n0 = len(pos)
        assert _ball(n0) == DELTA and _ball(n0 + len(batch)) == DELTA
        cand = drrt.extend_candidates(be.tree, be.S, batch, DELTA)
        self_ = drrt.extend_candidates_self(be.tree, be.S, batch, DELTA, skip=cand["sample_unsafe"])
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
            idx = np.concatenate([cand["idx"][a0:a1], mapped[keep]])
            assert (np.diff(idx) > 0).all()           # ascending node index, as the reference's list
            assert len(idx) > 0                       # (the closestNode rule is not part of the batched phase)
            cost = np.concatenate([cand["cost"][a0:a1], self_["cost"][s0:s1][keep]])
            hit_out = np.concatenate([cand["hit_out"][a0:a1], self_["hit_out"][s0:s1][keep]]).astype(bool)
            hit_in = np.concatenate([cand["hit_in"][a0:a1], self_["hit_in"][s0:s1][keep]]).astype(bool)
            n = len(pos)
            parent.append(-1); lmc.append(math.inf)
            bp, best = _adopt(idx, cost, hit_out, hit_in, lmc, parent, n)
            if bp < 0:
                parent.pop(); lmc.pop()
                continue
            node_of[j] = n
            pos.append(p); parent[n] = bp; lmc[n] = best
            inserted.append(drrt.RRTNode(p))
        drrt.kdInsertMany(be.tree, inserted)          # the batch's nodes in one rrtx_nodes_append
        assert be.tree.treeSize == len(pos) and [n.index for n in inserted] == list(range(n0, len(pos)))
    return np.array(pos), np.array(parent), np.array(lmc)


def test_batched_extend_grows_the_cpu_tree(oracle):
    sph = _spheres()
    rng = np.random.default_rng(SEED)
    samples = [rng.uniform(LO, HI, 3) for _ in range(N_ITER)]       # the samples _grow draws with this seed
    cpu = _RecordingCpu(oracle, sph)
    c = _grow(cpu, N_ITER, seed=SEED)
    # no sample of the batched phase has an empty ball on the oracle's side (the closestNode rule would need a nearest
    # search over the batch)
    assert cpu.it == N_ITER and all(n > 0 for it, n in cpu.lens if it > N_SEQ)
    g = _grow_batched(_GpuBackend(sph, 1), samples)
    assert len(g[0]) == len(c[0]) and len(g[0]) > 0.7 * N_ITER
    assert np.array_equal(g[0], c[0])
    assert np.array_equal(g[1], c[1])
    assert np.array_equal(g[2].view(np.uint64), c[2].view(np.uint64))            # bit-exact costs-to-goal
