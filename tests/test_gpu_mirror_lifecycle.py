"""One long-lived Context through what a planner does to the device mirror of its edges: the tree and the mirror grow
between bursts, sphere tables change length, obstacles arrive (rrtx_obstacle_sweep_batch, block) and leave
(rrtx_obstacle_release_batch, unblock), costs are re-priced, the mirror is cleared and refilled, and
rrtx_graph_cost_update resumes from the previous solve every time.  A host model of the mirror (mirror_model.py) takes
the same calls; after every step the device's rows, rrtLMC and parent edges are held against the oracle run on the
model's state with == / np.array_equal.  Nothing is read back from the device into the model.

The sequence is built once on the model alone (build_plan: a list of calls with what each must return, and the counts
the scene conditions are judged on) and replayed on the device by the gpu test."""
import ctypes as C

import numpy as np
import pytest

from mirror_model import INF, MirrorModel
from rrtqx_3d_amd import _capi
from rrtqx_3d_amd.context import Context
from test_gpu_graph_cost import _check_parents, _geometric_graph

ROOT = 0
RR1, RR2, DELTA = 0.5, 0.8, 8.0
N, BALL = 3100, 5.9                     # nodes, ball radius of the geometric graph
STAGES = (1880, 2250, 3100)             # nodes after the three appends
K1, K2, K3 = 150, 200, 100              # lengths of the three sphere tables
SEED = 2024


def _table(rng, K, pts):
    """A sphere table as the Scene of the batch test files generates it; a sphere that would swallow the root and with it
    every edge into the root is pushed off along x until the root is 1.5 clear of it (the solve must keep a tree)."""
    sph = np.concatenate([rng.uniform(-25, 25, (K, 3)), rng.uniform(1.0, 6.0, (K, 1))], 1)
    sph[3, :3] = pts[ROOT] + [2.0, 0.0, 0.0]               # an obstacle right at the root
    sph[K - 1] = (29.5, 29.5, -29.5, 0.05)                 # a tiny one in a corner
    for j in range(K):
        d = sph[j, :3] - pts[ROOT]
        need = sph[j, 3] + RR2 + 1.5
        if np.sqrt((d * d).sum()) < need:
            sph[j, :3] = pts[ROOT] + [need, 0.0, 0.0]
    return sph


def _lowest_parents(lmc, s, e, w):
    """the lowest edge id that attains each node's value (what the device reports), and how many edges attain it"""
    n = len(lmc)
    fin = np.isfinite(lmc)
    ok = np.isfinite(w) & fin[e] & fin[s] & (s != ROOT)
    att = np.flatnonzero(ok & (np.where(ok, lmc[e] + np.where(ok, w, 0.0), INF) == lmc[s]))
    lowest = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(lowest, s[att], att)
    lowest[lowest == np.iinfo(np.int64).max] = -1
    return lowest, np.bincount(s[att], minlength=n)


class Plan:
    """The calls, in order, as (op, arguments and expected results); the model they were run on; the counts."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.m = MirrorModel(oracle)
        self.steps = []
        self.cap = 0                                        # the mirror's capacity as rrtx_graph_edges_append grows it
        self.regrows = []                                   # (edges before, blocked before, capacity after)
        self.bursts = []                                    # one dict per sweep / release call
        self.solves = []                                    # one dict per solve
        self.hand = np.zeros(0, dtype=np.int32)             # ids the host blocked by hand that no sphere hits
        self.csr_ne = 0                                     # edges at the last full solve (the in-edge CSR holds these)
        self.swept_tail = np.zeros(0, dtype=np.int32)       # ids >= csr_ne a sweep blocked
        self.tail_released = 0
        self.notes = {}
        self.cnt = np.zeros(0, dtype=np.int64)              # the per-(obstacle, block) counts as the last calls left them
        self.stale_reads = []                               # per batched call: stale non-zero counts in blocks without a hit

    def _counts(self, rows):
        """What a batched call finds in the workspace it shares with the calls before it: its counts are laid out
        obstacle-major with the call's own number of 1024-edge blocks, and a block in which no edge hits any obstacle of
        the group has its counts zeroed on a path of its own.  Counts the places where that path meets a non-zero
        value an earlier call left (fresh memory is taken as zero)."""
        nb = -(-self.m.ne // 1024)
        met = 0
        for g in range(0, len(rows), 64):
            grp = rows[g:g + 64]
            need = len(grp) * nb
            if len(self.cnt) < need:
                self.cnt = np.concatenate([self.cnt, np.zeros(need - len(self.cnt), dtype=np.int64)])
            c = np.stack([np.bincount(np.asarray(r, dtype=np.int64) // 1024, minlength=nb) for r in grp])
            none = c.sum(0) == 0
            view = self.cnt[:need].reshape(len(grp), nb)
            met += int((view[:, none] != 0).sum())
            view[:, :] = c
        self.stale_reads.append(met)

    def add(self, op, **kw):
        self.steps.append((op, kw))
        return kw

    # ---- calls ----
    def nodes(self, pts):
        self.m.nodes_append(pts)
        self.add("nodes", pts=np.array(pts))

    def append(self, s, e):
        ne, n = self.m.ne, len(s)
        if ne + n > self.cap:
            nc = self.cap if self.cap > 0 else 4096
            while nc < ne + n:
                nc *= 2
            if ne > 0:
                self.regrows.append((ne, len(self.m.blocked), nc))
            self.cap = nc
        first = self.m.append(s, e)
        self.add("append", s=np.array(s, dtype=np.int32), e=np.array(e, dtype=np.int32), first=first)

    def set_dist(self, first, w):
        self.m.set_dist(first, w)
        self.add("set_dist", first=int(first), w=np.array(w, dtype=np.float64))

    def block(self, ids):
        ids = np.asarray(ids, dtype=np.int32)
        self.m.block(ids)
        self.add("block", ids=ids)

    def clear(self):
        self.m.clear()
        self.hand = self.hand[:0]
        self.swept_tail = self.swept_tail[:0]
        self.csr_ne = 0
        self.add("clear")

    def spheres_set(self, tab, active):
        self.m.spheres_set(tab, active)
        self.add("spheres_set", tab=np.array(tab), active=np.array(active, dtype=np.uint8))

    def obstacle_update(self, which, active):
        for j in np.atleast_1d(which):
            self.m.obstacle_update(int(j), float(self.m.cxyzr[j, 3]), active)
            self.add("obstacle_update", which=int(j), radius=float(self.m.cxyzr[j, 3]), active=bool(active))

    def _burst(self, kind, obs, **kw):
        b = dict(kind=kind, k=len(obs), m=len(self.m.cxyzr), in_use=int(self.m.active.sum()), ne=self.m.ne,
                 nb=-(-self.m.ne // 1024), **kw)
        self.bursts.append(b)
        return b

    def sweep(self, obs, search, rr, block, label):
        obs, search = np.asarray(obs, dtype=np.int32), np.asarray(search, dtype=np.float64)
        rows = [self.m.sweep_row(int(j), float(r), rr) for j, r in zip(obs, search)]
        allr = np.concatenate(rows) if len(rows) else np.zeros(0, dtype=np.int32)
        seen = np.bincount(allr, minlength=max(self.m.ne, 1))
        self._burst("sweep", obs, label=label, total=len(allr), empty=sum(len(r) == 0 for r in rows),
                    twice=int((seen >= 2).sum()))
        self._counts(rows)
        singles = sorted({0, len(obs) // 2, len(obs) - 1})
        self.add("sweep", obs=obs, search=search, rr=rr, block=block, rows=rows, singles=singles, label=label)
        if block:
            union = np.unique(allr)
            new = union[np.isfinite(self.m.dist[union])]
            self.swept_tail = np.union1d(self.swept_tail, new[new >= self.csr_ne]).astype(np.int32)
            self.m.block(union)
        return rows

    def release(self, obs, search, rr, unblock, label, stats=True):
        m = self.m
        obs, search = np.asarray(obs, dtype=np.int32), np.asarray(search, dtype=np.float64)
        rows = [m.release_row(int(j), float(r), rr, obs) for j, r in zip(obs, search)]
        allr = np.concatenate(rows)
        freed = np.unique(allr)
        blocked = m.blocked
        self._counts(rows)
        b = self._burst("release", obs, label=label, total=len(allr), freed=len(freed))
        stay = m.active.copy()
        stay[obs] = 0
        if stats:
            hits = [np.intersect1d(m.hits(int(j), float(r), rr), blocked) for j, r in zip(obs, search)]
            kept = np.unique(np.concatenate([np.setdiff1d(h, w) for h, w in zip(hits, rows)])).astype(np.int32)
            packed = m.packed_position()
            _, hm = m.hit_matrix_rows(kept, rr)                 # kept x table
            hm_stay = hm & (stay != 0)[None, :]
            assert hm_stay.any(1).all()                         # kept means: some staying sphere hits it
            lone = hm_stay.sum(1) == 1
            high = lone & (packed[np.argmax(hm_stay, 1)] >= 64)
            in_range = np.zeros(len(m.pts), dtype=bool)
            for j, r in zip(obs, search):
                in_range |= m.in_range(int(j), float(r)) != 0
            hand = self.hand[np.isinf(m.dist[self.hand])]
            hand = hand[in_range[m.start[hand]]]
            if len(hand):
                p0, p1 = m.pts[m.start[hand]], m.pts[m.end[hand]]
                anyhit, _ = self.oracle.edges_check_spheres(*self.oracle.make_spheres(m.cxyzr), p0, p1, rr)
                hand = hand[np.asarray(anyhit) == 0]
            b.update(kept=len(kept), kept_high=int(high.sum()), hand=len(hand), hand_freed=int(np.isin(hand, freed).sum()))
        # the documented relation to the single calls, for leaving positions that are in use
        act = [i for i in range(len(obs)) if m.active[obs[i]]]
        singles = sorted({act[0], act[len(act) // 2], act[-1]}) if act else []
        self.add("release", obs=obs, search=search, rr=rr, unblock=unblock, rows=rows, singles=singles,
                 blocked_before=blocked.copy(), stay=stay, label=label)
        if unblock:
            self.tail_released += int(np.isin(freed, self.swept_tail).sum())
            self.swept_tail = np.setdiff1d(self.swept_tail, freed).astype(np.int32)
            m.unblock(freed)
        return rows

    def fail(self, kind, obs, search, rr, rows):
        total = sum(len(r) for r in rows)
        self._counts(rows)
        self.add(kind + "_fail", obs=np.asarray(obs, dtype=np.int32), search=np.asarray(search, dtype=np.float64), rr=rr,
                 total=total, offsets=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64))

    def solve(self, kind, label, same_as=None):
        m = self.m
        lmc, par = m.solve(ROOT)
        lowest, natt = _lowest_parents(lmc, m.start, m.end, m.dist)
        fin = np.isfinite(lmc)
        fin[ROOT] = False
        if kind == "full" or self.csr_ne == 0:
            self.csr_ne = m.ne
        rec = dict(label=label, finite=int(fin.sum()), n=len(lmc), ties=int((natt[fin] > 1).sum()), lmc=lmc, lowest=lowest)
        self.solves.append(rec)
        self.add("solve", kind=kind, label=label, lmc=lmc, par=par, s=m.start.copy(), e=m.end.copy(), w=m.dist.copy(),
                 same_as=same_as)
        return rec

    # ---- choices the script makes on the model ----
    def unhit(self, ids, rr):
        """of the edge ids, those no sphere of the table hits, whatever its flag"""
        m = self.m
        hit, _ = self.oracle.edges_check_spheres(*self.oracle.make_spheres(m.cxyzr), m.pts[m.start[ids]], m.pts[m.end[ids]], rr)
        return ids[np.asarray(hit) == 0]

    def near(self, obs, search):
        mask = np.zeros(len(self.m.pts), dtype=bool)
        for j, r in zip(obs, search):
            mask |= self.m.in_range(int(j), float(r)) != 0
        return mask


def _range(tab, j, rr, extra=0.0):
    return rr + DELTA + tab[j, 3] + extra


def build_plan(oracle):
    rng = np.random.default_rng(SEED)
    P = Plan(oracle)
    m = P.m
    pts = rng.uniform(-30, 30, (N, 3))
    s_all, e_all = _geometric_graph(oracle, pts, BALL)
    born = np.maximum(s_all, e_all)                          # the tree grows in index order: an edge exists once both nodes do
    order = np.argsort(born, kind="stable")
    s_all, e_all, born = s_all[order], e_all[order], born[order]
    ne_at = [int(np.searchsorted(born, n)) for n in STAGES]
    P.notes["ne_at"] = ne_at

    # 1: stage 1, full solve
    P.nodes(pts[:STAGES[0]])
    P.append(s_all[:ne_at[0]], e_all[:ne_at[0]])
    P.solve("full", "1 stage 1")

    # 2: arrival burst A: 130 of the 150 spheres are in use and arrive at once (groups of 64, 64, 2), shuffled
    t1 = _table(rng, K1, pts)
    act = np.zeros(K1, dtype=np.uint8)
    act[:130] = 1
    P.spheres_set(t1, act)
    burst_a = rng.permutation(130).astype(np.int32)
    P.sweep(burst_a, [_range(t1, j, RR1) for j in burst_a], RR1, True, "2 burst A")
    P.solve("update", "2 burst A")

    # 3: stage 2 crosses a doubling of the mirror while edges are blocked; extend()'s own check blocks the new edges
    # that collide with a sphere in use
    P.nodes(pts[STAGES[0]:STAGES[1]])
    P.append(s_all[ne_at[0]:ne_at[1]], e_all[ne_at[0]:ne_at[1]])
    new = np.arange(ne_at[0], ne_at[1], dtype=np.int32)
    hit, _ = oracle.edges_check_spheres(*oracle.make_spheres(m.cxyzr, m.active), pts[s_all[new]], pts[e_all[new]], RR1)
    P.block(new[np.asarray(hit) != 0])
    P.solve("update", "3 stage 2")

    # 4: re-pricing in runs: cheaper, dearer, blocked edges given a finite cost, edges given Inf; a few blocked by hand
    free = np.flatnonzero(np.isfinite(m.dist)).astype(np.int32)
    pick = np.sort(rng.choice(free, 3000, replace=False))
    new_w = m.dist.copy()
    new_w[pick[0::2]] *= 0.25
    new_w[pick[1::2]] *= 3.0
    burst5 = rng.permutation(130)[:40].astype(np.int32)
    search5 = np.array([_range(t1, j, RR1, x) for j, x in zip(burst5, rng.uniform(0.0, 2.0, 40))])
    spare = np.arange(130, 150, dtype=np.int32)              # (step 6 brings these in and out again)
    spare_only = np.zeros(K1, dtype=np.uint8)
    spare_only[spare] = 1
    hit, _ = oracle.edges_check_spheres(*oracle.make_spheres(t1, spare_only), pts[m.start[m.blocked]], pts[m.end[m.blocked]], RR1)
    refin = rng.choice(m.blocked[np.asarray(hit) == 0], 40, replace=False)      # blocked -> finite: replaces distOriginal
    new_w[refin] = rng.uniform(0.5, 6.0, 40)
    cand = P.unhit(free[P.near(burst5, search5)[m.start[free]]], RR1)
    cand = rng.permutation(np.setdiff1d(cand, pick))
    to_inf, by_hand = np.sort(cand[:30]).astype(np.int32), np.sort(cand[30:60]).astype(np.int32)
    new_w[to_inf] = INF
    changed = np.sort(np.concatenate([pick, refin, to_inf]))
    for run in np.split(changed, np.flatnonzero(np.diff(changed) != 1) + 1):
        P.set_dist(int(run[0]), new_w[run])
    P.block(by_hand)
    P.hand = np.concatenate([to_inf, by_hand]).astype(np.int32)
    P.notes["repriced"] = (len(pick), len(refin), len(to_inf), len(by_hand))
    P.solve("update_dev", "4 re-priced")

    # 5: departure burst, 40 leave, its own range each; half of them already carry flag 0
    P.obstacle_update(burst5[::2], False)
    P.release(burst5, search5, RR1, True, "5 departure")
    P.obstacle_update(burst5[1::2], False)
    rec5 = P.solve("update", "5 departure")

    # 6: the 20 spare spheres arrive and leave again before any solve
    search6 = np.array([_range(t1, j, RR1) for j in spare])
    P.obstacle_update(spare, True)
    before = m.dist.copy()
    finite_before = np.isfinite(before)
    rows = P.sweep(spare, search6, RR1, True, "6 block")
    newly = np.unique(np.concatenate(rows))
    newly = newly[finite_before[newly]]
    rows = P.release(spare, search6, RR1, True, "6 unblock")
    both = np.intersect1d(newly, np.unique(np.concatenate(rows)))
    P.obstacle_update(spare, False)
    P.notes["step6"] = dict(both=len(both), parents=int(np.isin(both, rec5["lowest"]).sum()),
                            net_zero=bool(np.array_equal(before, m.dist)))
    P.solve("update", "6 block + unblock", same_as="5 departure")

    # 7: a longer table, another robot radius; burst B of 65, stage 3 across the next doubling, 64 of the 65 leave
    t2 = _table(rng, K2, pts)
    P.spheres_set(t2, np.ones(K2, dtype=np.uint8))
    burst_b = rng.permutation(K2)[:65].astype(np.int32)
    search_b = np.array([_range(t2, j, RR2) for j in burst_b])
    P.sweep(burst_b, search_b, RR2, True, "7 burst B")
    free = np.flatnonzero(np.isfinite(m.dist)).astype(np.int32)
    cand = P.unhit(free[P.near(burst_b, search_b)[m.start[free]]], RR2)
    hand7 = np.sort(rng.permutation(cand)[:30]).astype(np.int32)
    P.block(hand7)
    P.hand = np.concatenate([P.hand, hand7])
    P.solve("update", "7 burst B")
    P.nodes(pts[STAGES[1]:STAGES[2]])
    P.append(s_all[ne_at[1]:ne_at[2]], e_all[ne_at[1]:ne_at[2]])
    leave_b = burst_b[rng.permutation(65)[:64]]
    search_lb = np.array([_range(t2, j, RR2, x) for j, x in zip(leave_b, rng.uniform(0.0, 2.0, 64))])
    P.obstacle_update(leave_b[::3], False)
    P.release(leave_b, search_lb, RR2, True, "7 departure")
    P.obstacle_update(leave_b, False)
    P.solve("update", "7 stage 3 + departure")

    # 8: a call that runs out of room changes nothing: burst C of 30 spheres of the table nobody swept yet
    burst_c = np.setdiff1d(np.arange(K2, dtype=np.int32), burst_b)[:30].astype(np.int32)
    search_c = np.array([_range(t2, j, RR2) for j in burst_c])
    rows_c = [m.sweep_row(int(j), float(r), RR2) for j, r in zip(burst_c, search_c)]
    P.fail("sweep", burst_c, search_c, RR2, rows_c)
    P.solve("update", "8 failed sweep", same_as="7 stage 3 + departure")
    P.sweep(burst_c, search_c, RR2, True, "8 burst C")
    P.solve("update", "8 burst C")
    rows_r = [m.release_row(int(j), float(r), RR2, burst_c) for j, r in zip(burst_c, search_c)]
    P.fail("release", burst_c, search_c, RR2, rows_r)
    P.solve("update", "8 failed release", same_as="8 burst C")
    P.release(burst_c, search_c, RR2, True, "8 departure C")
    P.obstacle_update(burst_c, False)
    P.solve("update", "8 departure C")

    # 9: the mirror is cleared and refilled with the edges that start at an even node; a shorter table, 40 in use;
    # one sphere arrives, 50 more come into use, the one leaves
    P.clear()
    even = np.flatnonzero(s_all % 2 == 0)
    P.append(s_all[even], e_all[even])
    t3 = _table(rng, K3, pts)
    act = np.zeros(K3, dtype=np.uint8)
    # the one that arrives: of the first 40, the sphere with the most edges through it that exactly one other sphere of
    # the first 90 hits, that one at position 64 or later
    m.spheres_set(t3, np.ones(K3, dtype=np.uint8))
    score = []
    for j in range(40):
        row = m.sweep_row(j, _range(t3, j, RR2), RR2)
        _, hm = m.hit_matrix_rows(row, RR2)
        hm[:, j] = False
        hm = hm[:, :90]
        score.append(int(((hm.sum(1) == 1) & (np.argmax(hm, 1) >= 64)).sum()) if len(row) >= 60 else -1)
    one = int(np.argmax(score))
    act[:40] = 1
    P.spheres_set(t3, act)
    P.solve("update", "9 refilled")                            # nothing to resume from: a full solve
    s1 = [_range(t3, one, RR2)]
    P.sweep([one], s1, RR2, True, "9 one arrives")
    free = np.flatnonzero(np.isfinite(m.dist)).astype(np.int32)
    cand = P.unhit(free[P.near([one], s1)[m.start[free]]], RR2)
    hand9 = np.sort(rng.permutation(cand)[:20]).astype(np.int32)
    P.block(hand9)
    P.hand = hand9
    P.obstacle_update(np.arange(40, 90), True)
    P.release([one], s1, RR2, True, "9 one leaves")
    P.obstacle_update([one], False)
    P.solve("update", "9 one arrived and left")
    return P


@pytest.fixture(scope="module")
def plan(oracle):
    return build_plan(oracle)


def _crosses(seq, level):
    """(downward, upward) crossings of `level` along the sequence"""
    pairs = list(zip(seq[:-1], seq[1:]))
    return sum(a > level >= b for a, b in pairs), sum(a <= level < b for a, b in pairs)


def test_the_scene_offers_what_the_sequence_needs(plan):
    """Judged on the oracle and the model alone, before the device is touched.  Counts of this scene (3100 nodes, ball
    radius 5.9; 12 828 / 18 060 / 34 298 edges after the three appends, 17 070 after the clear):
    the mirror regrows at 12 828 edges with 3473 blocked (to 32 768) and at 18 060 with 6867 blocked (to 65 536);
    1024-edge blocks per call 13, 18, 34, 17; burst sizes in call order 130, 40, 20, 20, 65, 64, 30, 30, 1, 1 (the two
    calls that fail for room repeat the 30s); table lengths 150, 200, 100; spheres in use 130, 110, 200, 178, 136, 40, 90.
    Sweeps (ids in all rows / empty rows / edges in two rows): A 4706 / 33 / 912, step 6 1173 / 4 / 66, B 4606 / 6 / 633,
    C 4390 / 2 / 558, the single sphere 115 / 0 / 0.  Releases (freed / kept by a staying sphere / of those with one
    staying hitter, at a packed position >= 64 / hand-blocked in range that no sphere hits, none of them freed):
    step 5 1060 / 671 / 265 / 60, step 6 651 / 456 / 64 / 26, step 7 1976 / 1880 / 842 / 55, step 8 2705 / 1110 / 657 / 38,
    the single sphere 72 / 43 / 39 / 20.  Step 6 blocks and unblocks 651 edges between two updates, 92 of them parent
    edges of the solve before, every cost as it was.  2138 edges with ids beyond the in-edge CSR are blocked by a sweep
    and later released.  Blocks of 1024 edges without a hit meet non-zero counts of an earlier call or group in 6 of
    the 12 batched calls (8, 6, 10, 264, 2 and 1 counts).  No finite node has two edges that attain its value after any of the 14 solves."""
    P = plan
    sweeps = [b for b in P.bursts if b["kind"] == "sweep"]
    releases = [b for b in P.bursts if b["kind"] == "release"]
    for b in P.bursts:
        print(b)
    print("regrows (edges, blocked, new capacity):", P.regrows, "edges per stage:", P.notes["ne_at"], "re-priced:",
          P.notes["repriced"], "step 6:", P.notes["step6"], "tail released:", P.tail_released, "stale counts met:",
          P.stale_reads)
    print("solves:", [(s["label"], s["finite"], s["n"], s["ties"]) for s in P.solves])
    # the mirror grows across two doublings, one at least with edges blocked; the block count shrinks once
    assert len(P.regrows) >= 2 and sum(blk >= 100 for _, blk, _ in P.regrows) >= 1
    assert all(cap2 >= 2 * 4096 for _, _, cap2 in P.regrows)
    nbs = [b["nb"] for b in P.bursts]
    assert len(set(nbs)) >= 3 and sum(b < a for a, b in zip(nbs[:-1], nbs[1:])) == 1
    after_clear = [i for i, (op, _) in enumerate(P.steps) if op == "clear"]
    assert len(after_clear) == 1 and nbs[-1] < max(nbs)
    # burst sizes
    ks = [b["k"] for b in P.bursts]
    assert any(a > 64 and b < 64 for a, b in zip(ks[:-1], ks[1:])) and 64 in ks and 65 in ks and 1 in ks
    # the sphere table
    ms = [b["m"] for b in P.bursts]
    assert any(b > a for a, b in zip(ms[:-1], ms[1:])) and any(b < a for a, b in zip(ms[:-1], ms[1:]))
    down, up = _crosses([b["in_use"] for b in P.bursts], 64)
    assert down >= 1 and up >= 1
    # sweeps and releases
    assert all(b["total"] >= 50 for b in sweeps) and any(b["empty"] >= 1 for b in sweeps)
    assert any(b["twice"] >= 1 for b in sweeps)
    assert len(releases) >= 5
    for b in releases:
        assert b["freed"] >= 20 and b["kept"] >= 10 and b["kept_high"] >= 5 and b["hand"] >= 5 and b["hand_freed"] == 0, b
    # re-pricing: cheaper and dearer, blocked edges given a finite cost, edges given Inf, edges blocked by hand
    assert all(c >= 10 for c in P.notes["repriced"])
    # blocked and unblocked between two updates
    s6 = P.notes["step6"]
    assert s6["both"] >= 10 and s6["parents"] >= 3 and s6["net_zero"]
    # blocked and released beyond the CSR
    assert P.tail_released >= 10
    # a block of 1024 edges without a hit meets counts an earlier call or group left in the shared workspace
    assert sum(c > 0 for c in P.stale_reads) >= 3 and sum(P.stale_reads) >= 10
    # the solves keep a tree, and ties cannot hide a parent
    for s in P.solves:
        assert s["finite"] >= s["n"] // 3 and s["ties"] <= 0.01 * s["finite"], s
    kinds = [a["kind"] for op, a in P.steps if op == "solve"]
    assert kinds[0] == "full" and "update_dev" in kinds and kinds.count("update") >= 8


def _rows_of(off, ids):
    assert off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    return [ids[off[j]:off[j + 1]] for j in range(len(off) - 1)]


def _check_rows(off, ids, want, label):
    assert off.dtype == np.int64 and ids.dtype == np.int32 and len(off) == len(want) + 1, label
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])])), label
    for j, row in enumerate(_rows_of(off, ids)):
        assert np.array_equal(row, want[j]), (label, j)


def _check_solve(lmc, par, a):
    assert np.array_equal(lmc, a["lmc"]), a["label"]
    att = _check_parents(lmc, par, a["s"], a["e"], a["w"], ROOT)
    single = np.bincount(a["s"][att], minlength=len(lmc)) == 1      # the reference breaks ties by visiting order
    assert np.array_equal(par[single], a["par"][single]), a["label"]


@pytest.mark.gpu
def test_one_context_follows_the_model_through_the_sequence(plan):
    """Every call of the plan on one Context, every result against what the model says: rows and offsets of the sweeps
    and releases, rrtLMC bit for bit and parent edges after every solve (host form, and rrtx_graph_cost_update_dev
    into torch buffers once), the calls that fail for room, the clear; at the end a fresh context given the model's
    final edges and costs solves to the same answer."""
    torch = pytest.importorskip("torch")
    P = plan
    es, ee = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)    # what the host appended (not read back)
    solved = {}
    with Context(3) as ctx:
        for op, a in P.steps:
            if op == "nodes":
                ctx.nodes_append(a["pts"])
            elif op == "append":
                assert ctx.graph_edges_append(a["s"], a["e"]) == a["first"]
                es, ee = np.concatenate([es, a["s"]]), np.concatenate([ee, a["e"]])
                assert ctx.n_graph_edges == len(es)
            elif op == "set_dist":
                ctx.graph_edges_set_dist(a["first"], a["w"])
            elif op == "block":
                ctx.graph_edges_block(a["ids"])
            elif op == "clear":
                ctx.graph_edges_clear()
                es, ee = es[:0], ee[:0]
                assert ctx.n_graph_edges == 0
            elif op == "spheres_set":
                ctx.spheres_set(a["tab"], a["active"])
            elif op == "obstacle_update":
                ctx.obstacle_update(a["which"], a["radius"], a["active"])
            elif op == "sweep":
                total = sum(len(r) for r in a["rows"])
                off, ids = ctx.obstacle_sweep_batch(a["obs"], a["search"], a["rr"], block=a["block"], cap=total)
                _check_rows(off, ids, a["rows"], a["label"])
                for j in a["singles"]:                               # row j is the single call
                    one = ctx.obstacle_sweep(int(a["obs"][j]), float(a["search"][j]), a["rr"])
                    assert np.array_equal(one, a["rows"][j]), (a["label"], j)
            elif op == "release":
                total = sum(len(r) for r in a["rows"])
                off, ids = ctx.obstacle_release_batch(a["obs"], a["search"], a["rr"], unblock=a["unblock"], cap=total)
                _check_rows(off, ids, a["rows"], a["label"])
                for j in a["singles"]:                               # row j from the single calls, for a sphere in use
                    one = ctx.obstacle_sweep(int(a["obs"][j]), float(a["search"][j]), a["rr"])
                    one = one[np.isin(one, a["blocked_before"])]
                    if len(one):
                        hit, _ = ctx.edges_check_idx(es[one], ee[one], a["rr"], obstacle=-1, obstacle_mask=a["stay"],
                                                     want_first=False)
                        one = one[hit == 0]
                    assert np.array_equal(one, a["rows"][j]), (a["label"], j)
            elif op in ("sweep_fail", "release_fail"):
                k, total = len(a["obs"]), a["total"]
                assert total >= 2
                off = np.zeros(k + 1, dtype=np.int64)
                ids = np.empty(total, dtype=np.int32)
                needed = C.c_int64()
                fn = ctx._lib.rrtx_obstacle_sweep_batch if op == "sweep_fail" else ctx._lib.rrtx_obstacle_release_batch
                rc = fn(ctx.handle, _capi._ptr(a["obs"]), k, _capi._ptr(a["search"]), a["rr"], 1, _capi._ptr(off),
                        _capi._ptr(ids), total - 1, C.byref(needed))
                assert rc == _capi.RRTX_E_CAPACITY and needed.value == total
                assert np.array_equal(off, a["offsets"])
            elif op == "solve":
                if a["kind"] == "update_dev":
                    n = ctx.n_nodes
                    d_lmc = torch.empty(n, dtype=torch.float64, device="cuda:0")
                    d_par = torch.empty(n, dtype=torch.int32, device="cuda:0")
                    torch.cuda.synchronize()
                    ctx.graph_cost_update_dev(ROOT, d_lmc.data_ptr(), d_par.data_ptr())
                    ctx.sync()
                    lmc, par = d_lmc.cpu().numpy(), d_par.cpu().numpy()
                    _check_solve(lmc, par, a)
                    lmc_h, par_h, _ = ctx.graph_cost_update(ROOT)   # the host form on the same state
                    assert np.array_equal(lmc_h, lmc) and np.array_equal(par_h, par)
                else:
                    fn = ctx.graph_cost_to_root if a["kind"] == "full" else ctx.graph_cost_update
                    lmc, par, _ = fn(ROOT)
                    _check_solve(lmc, par, a)
                if a["same_as"] is not None:
                    lmc0, par0 = solved[a["same_as"]]
                    assert np.array_equal(lmc, lmc0) and np.array_equal(par, par0), a["label"]
                solved[a["label"]] = (lmc, par)
            else:
                raise AssertionError(op)
        # the same mirror from nothing
        m = P.m
        with Context(3) as fresh:
            fresh.nodes_append(m.pts)
            assert fresh.graph_edges_append(m.start, m.end) == 0
            fresh.graph_edges_set_dist(0, m.dist)
            lmc_f, par_f, _ = fresh.graph_cost_to_root(ROOT)
        assert np.array_equal(lmc_f, lmc) and np.array_equal(par_f, par)
