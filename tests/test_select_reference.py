"""The reference for the selection step (findBestParent, R/DRRT_Q.jl:1927-1979, and the rewire test of extend,
:2619-2634) that the GPU tests compare against: `select_numpy`, a vectorised restatement of the three rules of
include/rrtx.h, held here against `select_loop`, the literal per-sample loop of tests/test_gpu_planner_loop.py's
_grow.  Neither touches the product: lists in, answers out, numpy only."""
import math

import numpy as np

SEL_OK, SEL_NO_PARENT, SEL_EMPTY, SEL_UNSAFE, SEL_OVERFLOW = 0, 1, 2, 3, 4
KEYS = ("status", "parent_idx", "parent_entry", "lmc_new", "rw_offsets", "rw_node", "rw_value")


def select_loop(offsets, idx, cost_out, cost_in, hit_out, hit_in, unsafe, lmc, root_skip=False):
    """_grow's two loops, per sample.  root_skip keeps its `j == 0` skip of the rewire loop (the reference never rewires
    the root); with lmc[0] == 0 and non-negative costs it changes nothing, which a test below holds."""
    nq = len(offsets) - 1
    status = np.zeros(nq, dtype=np.uint8)
    parent_idx = np.full(nq, -1, dtype=np.int32)
    parent_entry = np.full(nq, -1, dtype=np.int64)
    lmc_new = np.full(nq, math.inf)
    rw_offsets = np.zeros(nq + 1, dtype=np.int64)
    rw_node, rw_value = [], []
    for s in range(nq):
        rw_offsets[s] = len(rw_node)
        if unsafe is not None and unsafe[s]:
            status[s] = SEL_UNSAFE
            continue
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if lo == hi:
            status[s] = SEL_EMPTY
            continue
        best, best_parent, best_e = math.inf, -1, -1
        for e in range(lo, hi):                                                 # findBestParent
            j, c, blocked = idx[e], cost_out[e], hit_out[e] != 0
            if not blocked and best > lmc[j] + c:
                best, best_parent, best_e = lmc[j] + c, int(j), e
        if best_parent < 0:
            status[s] = SEL_NO_PARENT
            continue
        status[s] = SEL_OK
        parent_idx[s], parent_entry[s], lmc_new[s] = best_parent, best_e, best
        for e in range(lo, hi):                                                 # one-hop rewire
            j, c, blocked = idx[e], cost_in[e], hit_in[e] != 0
            if blocked or (root_skip and j == 0):
                continue
            if lmc[j] > best + c and best_parent != j:
                rw_node.append(int(j))
                rw_value.append(best + c)
    rw_offsets[nq] = len(rw_node)
    return dict(status=status, parent_idx=parent_idx, parent_entry=parent_entry, lmc_new=lmc_new, rw_offsets=rw_offsets,
                rw_node=np.array(rw_node, dtype=np.int32), rw_value=np.array(rw_value, dtype=np.float64))


def select_numpy(offsets, idx, cost_out, cost_in, hit_out, hit_in, unsafe, lmc):
    """The same answers from segment reductions: the minimum of a segment by np.minimum.reduceat, its winner as the
    first position that attains it."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nq = len(offsets) - 1
    n = int(offsets[-1])
    idx, cost_out, cost_in = idx[:n], cost_out[:n], cost_in[:n]
    hit_out, hit_in = hit_out[:n], hit_in[:n]
    cnt = np.diff(offsets)
    seg = np.repeat(np.arange(nq), cnt)
    uns = np.zeros(nq, dtype=bool) if unsafe is None else np.asarray(unsafe) != 0
    full = cnt > 0
    starts = offsets[:-1][full]
    with np.errstate(invalid="ignore"):
        cand = lmc[idx] + cost_out
        usable = (hit_out == 0) & (cand < math.inf)              # NaN compares false: never adopted
    key = np.where(usable, cand, math.inf)
    best = np.full(nq, math.inf)
    first = np.full(nq, n, dtype=np.int64)
    if n:
        best[full] = np.minimum.reduceat(key, starts)
        attains = usable & (key == best[seg])
        first[full] = np.minimum.reduceat(np.where(attains, np.arange(n), n), starts)
    ok = (first < n) & ~uns
    status = np.where(uns, SEL_UNSAFE, np.where(~full, SEL_EMPTY, np.where(ok, SEL_OK, SEL_NO_PARENT))).astype(np.uint8)
    parent_entry = np.where(ok, first, -1).astype(np.int64)
    parent_idx = np.where(ok, idx[np.minimum(first, max(n - 1, 0))] if n else -1, -1).astype(np.int32)
    lmc_new = np.where(ok, best, math.inf)
    with np.errstate(invalid="ignore"):
        value = lmc_new[seg] + cost_in
        take = ok[seg] & (hit_in == 0) & (idx != parent_idx[seg]) & (lmc[idx] > value)
    rw_offsets = np.concatenate([[0], np.cumsum(np.bincount(seg[take], minlength=nq))]).astype(np.int64)
    return dict(status=status, parent_idx=parent_idx, parent_entry=parent_entry, lmc_new=lmc_new, rw_offsets=rw_offsets,
                rw_node=idx[take].astype(np.int32), rw_value=value[take])


def assert_same(a, b, what=""):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def tie_samples(offsets, idx, cost_out, hit_out, lmc):
    """Samples whose minimum is attained by two or more usable entries."""
    n = int(offsets[-1])
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    with np.errstate(invalid="ignore"):
        cand = lmc[idx[:n]] + cost_out[:n]
        usable = (hit_out[:n] == 0) & (cand < math.inf)
    best = np.full(len(offsets) - 1, math.inf)
    np.minimum.at(best, seg[usable], cand[usable])
    hits = np.bincount(seg[usable & (cand == best[seg])], minlength=len(offsets) - 1)
    return int((hits >= 2).sum())


def random_lists(rng, nq, n_nodes, mean_len, lattice=False, p_hit=0.2, p_unsafe=0.05, orphans=0.05, nan_at=None,
                 asymmetric=False):
    """Lists with the shape the extend preamble writes: per sample ascending distinct node indices."""
    cnt = rng.poisson(mean_len, nq)
    cnt[rng.random(nq) < 0.05] = 0
    cnt[rng.random(nq) < 0.05] = 1
    cnt = np.minimum(cnt, n_nodes)
    if nq:
        cnt[rng.integers(nq)] = min(n_nodes, 8 * mean_len + 70)    # one list longer than a wave
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(n_nodes, c, replace=False)) for c in cnt] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    n = len(idx)
    draw = (lambda m, hi: rng.integers(0, 4 * hi, m) / 4.0) if lattice else (lambda m, hi: rng.uniform(0.0, hi, m))
    cost_out = draw(n, 3)
    cost_in = draw(n, 3) if asymmetric else cost_out
    hit_out = (rng.random(n) < p_hit).astype(np.uint8) * rng.choice(np.array([1, 2, 3], dtype=np.uint8), n)
    hit_in = (rng.random(n) < p_hit).astype(np.uint8) * rng.choice(np.array([1, 2, 3], dtype=np.uint8), n)
    unsafe = (rng.random(nq) < p_unsafe).astype(np.uint8)
    lmc = draw(n_nodes, 10)
    lmc[rng.random(n_nodes) < orphans] = math.inf
    lmc[0] = 0.0
    if nan_at is not None:
        lmc[nan_at] = math.nan
    return offsets, idx, cost_out, cost_in, hit_out, hit_in, unsafe, lmc


def test_restatement_equals_the_loop_on_random_lists():
    rng = np.random.default_rng(11)
    seen = set()
    for trial in range(12):
        L = random_lists(rng, nq=int(rng.integers(1, 400)), n_nodes=int(rng.integers(300, 3000)), mean_len=int(rng.integers(1, 40)),
                         p_hit=[0.2, 0.9][trial % 2], nan_at=5 if trial % 3 == 0 else None, asymmetric=trial % 4 == 1)
        a, b = select_loop(*L), select_numpy(*L)
        assert_same(a, b, trial)
        seen |= set(a["status"].tolist())
    assert seen == {SEL_OK, SEL_NO_PARENT, SEL_EMPTY, SEL_UNSAFE}


def test_restatement_equals_the_loop_where_ties_decide():
    rng = np.random.default_rng(12)
    L = random_lists(rng, nq=600, n_nodes=2000, mean_len=25, lattice=True)
    assert tie_samples(L[0], L[1], L[2], L[4], L[7]) >= 16
    a, b = select_loop(*L), select_numpy(*L)
    assert_same(a, b)
    assert len(a["rw_node"]) > 0 and (a["status"] == SEL_OK).sum() > 300


def test_the_root_needs_no_special_case():
    """_grow skips j == 0 in its rewire loop; with lmc[root] == 0 and non-negative costs the rule never selects it."""
    rng = np.random.default_rng(13)
    for lattice in (False, True):
        L = random_lists(rng, nq=300, n_nodes=400, mean_len=30, lattice=lattice)
        assert (L[1] == 0).sum() > 5
        assert_same(select_loop(*L), select_loop(*L, root_skip=True))


def test_degenerate_inputs():
    z64, z32, zf, zu = np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0, dtype=np.uint8)
    out = select_numpy(z64, z32, zf, zf, zu, zu, zu, np.zeros(3))
    assert_same(out, select_loop(z64, z32, zf, zf, zu, zu, zu, np.zeros(3)))
    assert len(out["status"]) == 0 and out["rw_offsets"].tolist() == [0]
    # every candidate is +Inf or NaN, or every edge is blocked: no parent; -Inf is an ordinary (winning) value
    off = np.array([0, 2, 4, 6], dtype=np.int64)
    idx = np.array([0, 1, 0, 1, 2, 3], dtype=np.int32)
    cost = np.ones(6)
    lmc = np.array([math.inf, math.nan, -math.inf, 1.0])
    hit = np.array([0, 0, 1, 2, 0, 0], dtype=np.uint8)
    nohit = np.zeros(6, dtype=np.uint8)
    out = select_numpy(off, idx, cost, cost, hit, nohit, None, lmc)
    assert_same(out, select_loop(off, idx, cost, cost, hit, nohit, None, lmc))
    assert out["status"].tolist() == [SEL_NO_PARENT, SEL_NO_PARENT, SEL_OK] and out["parent_idx"][2] == 2
