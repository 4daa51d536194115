"""The batched planner loop of tests/test_gpu_planner_loop_batched.py from the root alone (no one-sample phase): every
sample goes through in batches of 64 -- drrt.extend_candidates (the lists against the tree as it stood),
drrt.extend_candidates_self (the batch among itself) and drrt.extend_closest_self (the closestNode rule: a sample whose
merged list is empty is linked to kdFindNearest over the tree as sequential insertion would have it, which may be an
earlier sample of its own batch).  The tree must equal, bit for bit, the one the CPU oracle grows one sample at a time.
What the scenes are there for -- empty balls, closest nodes in the own batch, safe samples that are not inserted,
closest nodes that are not the nearest live earlier sample, exhausted rows -- is counted from the CPU run."""
import math

import numpy as np
import pytest

import extend_closest_model as M
from rrtqx_3d_amd import drrt, synth
from test_gpu_planner_loop import DELTA, HI, LO, ROBOT_RADIUS, _CpuBackend, _GpuBackend, _grow, _spheres
from test_gpu_planner_loop_batched import _adopt, _ball

pytestmark = pytest.mark.gpu
BATCH = 64
SPH_ITER, SPH_SEED, SPH_ROOT = 1200, 7, np.array([15.0, 15.0, 15.0])
POLY_N, POLY_SEED, POLY_ITER, POLY_SAMPLE_SEED, POLY_R, POLY_RR = 24, 12, 600, 11, 1.0, 0.25
POLY_ROOT = np.array([0.0, 0.0, 0.0])


def _polygons():
    out = []
    for p in synth.polygons(POLY_N, seed=POLY_SEED):
        p = p * (10.0 / synth.WORLD)
        c = p.mean(axis=0)
        out.append(c + (p - c) * 0.6)
    return out


def _poly_samples():
    rng = np.random.default_rng(POLY_SAMPLE_SEED)
    return [np.array([*rng.uniform(-10.0, 10.0, 2), 0.0]) for _ in range(POLY_ITER)]


class _Recording:
    """mixin for a CPU backend: per iteration (nearest() opens one) the tree size, the nearest node, whether the sample
    is unsafe, the length of its list and the node it became (-1: none)"""

    def nearest(self, pos):
        self.log.append(dict(p=np.array(pos), size=len(self.pts), near=-1, unsafe=True, n_list=-1, node=-1))
        out = super().nearest(pos)
        self.log[-1]["near"] = int(out[0])
        return out

    def unsafe(self, pos):
        u = super().unsafe(pos)
        self.log[-1]["unsafe"] = bool(u)
        return u

    def candidates(self, pos, r):
        out = super().candidates(pos, r)
        self.log[-1]["n_list"] = len(out[0])
        return out

    def insert(self, pos):
        i = super().insert(pos)
        if self.log:                                   # (the root goes in before the first iteration)
            self.log[-1]["node"] = int(i)
        return i


class _SphereCpu(_Recording, _CpuBackend):
    def __init__(self, oracle, sph):
        super().__init__(oracle, sph)
        self.log = []


class _PolygonCpu(_Recording, _CpuBackend):
    def __init__(self, oracle):
        self.o, self.tree, self.ps = oracle, oracle.KDTree(3), oracle.PolygonSet(_polygons())
        self.pts, self.log = [], []

    def unsafe(self, pos):
        u = bool(self.o.point_check_polygons(self.ps, pos, POLY_RR)[0])
        self.log[-1]["unsafe"] = u
        return u

    def candidates(self, pos, r):
        idx, key = self.tree.within_range(r, pos)
        order = np.argsort(idx, kind="stable")
        idx, key = idx[order], key[order]
        self.log[-1]["n_list"] = len(idx)
        if len(idx) == 0:
            z = np.zeros(0, dtype=bool)
            return idx, key, z, z
        P = np.array([self.pts[i] for i in idx])
        Q = np.repeat(np.array([pos]), len(idx), 0)
        ho, _ = self.o.edges_check_polygons(self.ps, Q, P, POLY_RR)
        hi, _ = self.o.edges_check_polygons(self.ps, P, Q, POLY_RR)
        return idx, key, ho.astype(bool), hi.astype(bool)

    def edge_blocked(self, p0, p1):
        return bool(self.o.edges_check_polygons(self.ps, np.array([p0]), np.array([p1]), POLY_RR)[0][0])


class _PolygonGpu(_GpuBackend):
    def __init__(self):
        self.tree = drrt.KDTree(3)
        self.S = drrt.CSpace(3, 0.0, [-10.0, -10.0, 0.0], [10.0, 10.0, 0.0], [0, 0, 0], [0, 0, 0])
        self.S.robotRadius = POLY_RR
        self.S.bind(self.tree)
        for poly in _polygons():
            drrt.addObsToCSpace(self.S, drrt.Obstacle(3, poly))
        self.nodes = []


def _grow_seq(be, samples, root, ball):
    """_grow of tests/test_gpu_planner_loop.py over given samples, root and ball radius"""
    pos, parent, lmc = [root], [-1], [0.0]
    be.insert(root)
    for p in samples:
        near, _ = be.nearest(p)
        if be.unsafe(p):
            continue
        n = len(pos)
        idx, cost, hit_out, hit_in = be.candidates(p, ball(n))
        if len(idx) == 0:                                            # the closestNode rule (R/DRRT_Q.jl:1930-1935)
            idx = np.array([near])
            cost = np.array([be.dist(p, pos[near])])
            hit_out = np.array([be.edge_blocked(p, pos[near])])
            hit_in = np.array([be.edge_blocked(pos[near], p)])
        parent.append(-1); lmc.append(math.inf)                      # (slot n, dropped again without a parent)
        bp, best = _adopt(idx, cost, hit_out, hit_in, lmc, parent, n)
        if bp < 0:
            parent.pop(); lmc.pop()
            continue
        assert be.insert(p) == n
        pos.append(p); parent[n] = bp; lmc[n] = best
    return np.array(pos), np.array(parent), np.array(lmc)


def _rule_figures(log, pos, k):
    """From the CPU run (its log and the positions of its nodes), per batch of BATCH iterations: the samples with an
    empty ball, those whose closest node is a sample of their own batch, the rank of that sample among the live earlier
    ones by (s, i), the safe samples that were not inserted, and the rows a list of k exhausts: a live sample with an
    empty ball, at least k live earlier samples, none of the first k inserted, and the k-th nearer than the nearest
    node of the tree as it stood when the batch began (otherwise no later entry can beat that node)."""
    fig = dict(empty=0, own_batch=0, ranks=[], safe_not_inserted=0, exhausted=0)
    for b0 in range(0, len(log), BATCH):
        rows = log[b0:b0 + BATCH]
        first = rows[0]["size"]
        Q = np.array([e["p"] for e in rows])
        ranked = M.ranked_rows(Q, skip=[e["unsafe"] for e in rows])
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
                to_tree = np.sqrt(M.sq3_all(np.vstack([e["p"][None], pos[:first]]))[0, 1:].min())
                fig["exhausted"] += bool(np.sqrt(ranked[j][1][k - 1]) < to_tree)
            if e["near"] >= first:
                fig["own_batch"] += 1
                fig["ranks"].append(order.index(sample_of[e["near"]]))
    return fig


def _grow_batched(be, samples, root, ball, k):
    """every sample in batches from the root alone; returns the tree and the number of exhausted rows"""
    pos, parent, lmc = [root], [-1], [0.0]
    be.insert(root)
    exhausted = used_rule = 0
    for b0 in range(0, len(samples), BATCH):
        batch = np.array(samples[b0:b0 + BATCH])
        n0 = len(pos)
        r = ball(n0)
        assert r == ball(n0 + len(batch))
        cand = drrt.extend_candidates(be.tree, be.S, batch, r)
        unsafe = cand["sample_unsafe"]
        self_ = drrt.extend_candidates_self(be.tree, be.S, batch, r, skip=unsafe)
        want = ((np.diff(cand["offsets"]) == 0) & (unsafe == 0)).astype(np.uint8)
        clo = drrt.extend_closest_self(be.tree, be.S, batch, k, skip=unsafe, want=want, treeNearest=cand["nearest_idx"])
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
            cost = np.concatenate([cand["cost"][a0:a1], self_["cost"][s0:s1][keep]])
            hit_out = np.concatenate([cand["hit_out"][a0:a1], self_["hit_out"][s0:s1][keep]]).astype(bool)
            hit_in = np.concatenate([cand["hit_in"][a0:a1], self_["hit_in"][s0:s1][keep]]).astype(bool)
            if len(idx) == 0:                          # the closestNode rule
                assert want[j]
                used_rule += 1
                tree_link = (cand["nearest_idx"][j], cand["nearest_dist"][j], clo["tree_hit_out"][j], clo["tree_hit_in"][j])
                link = tree_link
                row = clo["idx"][j, :clo["count"][j]]
                ins = np.flatnonzero(node_of[row] >= 0)
                if len(ins):                           # the first entry whose sample was inserted
                    s = ins[0]
                    if clo["cost"][j, s] < cand["nearest_dist"][j]:
                        link = (node_of[row[s]], clo["cost"][j, s], clo["hit_out"][j, s], clo["hit_in"][j, s])
                elif clo["count"][j] == k and clo["cost"][j, k - 1] < cand["nearest_dist"][j]:
                    # exhausted: none of the k was inserted and a later entry may still beat the tree node; brute force
                    # over the batch, two edge checks
                    exhausted += 1
                    earlier = np.flatnonzero(node_of[:j] >= 0)
                    if len(earlier):
                        s_all = M.sq3_all(batch[:j + 1])[j, earlier]
                        i = earlier[np.lexsort((earlier, s_all))[0]]
                        c = np.sqrt(M.sq3_all(batch[[j, i]])[0, 1])
                        if c < cand["nearest_dist"][j]:
                            link = (node_of[i], c, be.edge_blocked(p, batch[i]), be.edge_blocked(batch[i], p))
                idx, cost = np.array([link[0]]), np.array([link[1]])
                hit_out, hit_in = np.array([bool(link[2])]), np.array([bool(link[3])])
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
    return (np.array(pos), np.array(parent), np.array(lmc)), exhausted, used_rule


def _same_tree(g, c):
    assert len(g[0]) == len(c[0])
    assert np.array_equal(g[0], c[0])
    assert np.array_equal(g[1], c[1])
    assert np.array_equal(g[2].view(np.uint64), c[2].view(np.uint64))            # bit-exact costs-to-goal


def test_spheres_from_the_root_alone(oracle):
    sph = _spheres()
    rng = np.random.default_rng(SPH_SEED)
    samples = [rng.uniform(LO, HI, 3) for _ in range(SPH_ITER)]      # the samples _grow draws with this seed
    cpu = _SphereCpu(oracle, sph)
    c = _grow(cpu, SPH_ITER, seed=SPH_SEED)
    assert len(cpu.log) == SPH_ITER and all(np.array_equal(e["p"], p) for e, p in zip(cpu.log, samples))
    fig = _rule_figures(cpu.log, c[0], 8)
    print(f"spheres: {fig['empty']} empty balls, {fig['own_batch']} closest nodes in the own batch, ranks "
          f"{sorted(set(fig['ranks']))}, {fig['safe_not_inserted']} safe samples not inserted, {fig['exhausted']} exhausted")
    assert fig["empty"] >= 10 and fig["own_batch"] >= 5              # the rule ran, with an own-batch closest node
    g, exhausted, used_rule = _grow_batched(_GpuBackend(sph, 1), samples, SPH_ROOT, _ball, 8)
    assert _ball(1) == DELTA and ROBOT_RADIUS == 0.5
    assert used_rule == fig["empty"] and exhausted == fig["exhausted"]
    assert len(g[0]) > 0.7 * SPH_ITER
    _same_tree(g, c)


@pytest.fixture(scope="module")
def polygon_cpu_run(oracle):
    cpu = _PolygonCpu(oracle)
    tree = _grow_seq(cpu, _poly_samples(), POLY_ROOT, lambda n: POLY_R)
    return cpu.log, tree


@pytest.mark.parametrize("k", [8, 4])
def test_polygons_from_the_root_alone(polygon_cpu_run, k):
    log, c = polygon_cpu_run
    assert len(log) == POLY_ITER
    fig = _rule_figures(log, c[0], k)
    hist = {r: fig["ranks"].count(r) for r in sorted(set(fig["ranks"]))}
    print(f"polygons, k = {k}: {fig['empty']} empty balls, {fig['own_batch']} closest nodes in the own batch, ranks {hist}, "
          f"{fig['safe_not_inserted']} safe samples not inserted, {fig['exhausted']} exhausted rows")
    assert fig["safe_not_inserted"] > 0                               # some safe samples are not inserted
    assert fig["own_batch"] > 0 and max(fig["ranks"]) > 0             # ... and ranks above 0 occur
    if k == 8:
        assert fig["exhausted"] == 0 and max(fig["ranks"]) < 8
    else:
        assert fig["exhausted"] >= 1
    g, exhausted, used_rule = _grow_batched(_PolygonGpu(), _poly_samples(), POLY_ROOT, lambda n: POLY_R, k)
    # the exit serves exactly the rows the list cannot: none is swallowed, none is invented
    assert used_rule == fig["empty"] and exhausted == fig["exhausted"]
    _same_tree(g, c)
