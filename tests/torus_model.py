"""Lattice tori for the wrapped searches, and the ghost rule of R/ghostPoint.jl:32-111 restated in plain numpy -- no
device and no oracle.  Up to three wrapped dimensions, so up to eight copies of a query:

  * copy k shifts the wrapped dimensions whose bit is set in k, the FIRST wrap set being the most significant bit;
  * a shifted coordinate p goes to p + period when p < period / 2 (strictly), else to p - period; the "closest unwrapped
    point" has period resp. 0 there;
  * copy k > 0 is skipped when sqrt(sq(closest, ghost)) > r (equal: searched);
  * a node is listed by the first copy with sqrt(sq(copy, node)) < r and keeps that copy's key; node 0, the root, is
    listed by copy 0 alone with <=;
  * squared distances are accumulated coordinate by coordinate, left to right.

Every coordinate is a multiple of 1/4 (theta of D4: of pi / 4) and the radii are lattice distances, so queries sit exactly
on period / 2, ghosts exactly on the skip threshold and nodes exactly at r.  tests/test_torus_scenes.py holds the oracle
to this restatement and the scenes to the cases they are there for; tests/test_gpu_torus.py and tools/soak_torus.py
compare the device with the oracle on them."""
import functools
import math

import numpy as np

TWO_PI = 2.0 * math.pi
RADII = (1.25, 2.5, 3.25, 3.75)          # 3-4-5 and 5-12-13 triples in quarters (thr_first_ge)
# name: dim, wrapped dimensions in set_wrap order (= copy order), their periods, span of the unwrapped dimensions,
# nodes drawn, queries.  T3r is T3 with the wraps set in another order: same nodes, same queries.
SPACES = {
    "T3": dict(dim=3, wraps=(0, 1, 2), periods=(8.0, 4.0, 8.0), span=4.0, n=4000, nq=256, seed=0),
    "T3r": dict(dim=3, wraps=(2, 0, 1), periods=(8.0, 8.0, 4.0), span=4.0, n=4000, nq=256, seed=0),
    "T2": dict(dim=3, wraps=(0, 2), periods=(8.0, 4.0), span=4.0, n=4000, nq=256, seed=1),
    "T4": dict(dim=4, wraps=(0, 2, 3), periods=(8.0, 4.0, 8.0), span=2.0, n=4000, nq=256, seed=2),
    # D4's only lattice period is 4, where a ghost sits exactly on the skip threshold for r = 1.25 alone (t = 1.25 or
    # 2.75): on_skip of its queries of that radius are put there (_plant_on_skip)
    "D4": dict(dim=4, wraps=(3, 2), periods=(TWO_PI, 4.0), span=5.0, n=900, nq=128, seed=3, on_skip=20),
    # Two copies that shift different dimensions reach one node only when sqrt(p_a^2 + p_b^2) < 2 r: never with
    # periods 8 and 4 and r < 4, so T3 and T3r hold exactly the same keys.  Two periods of 4 (5.66 < 2 * 3.25) make
    # the order of the wraps decide which copy finds a node first: T3s and T3sr differ in keys.
    "T3s": dict(dim=3, wraps=(0, 1, 2), periods=(4.0, 4.0, 8.0), span=4.0, n=2500, nq=128, seed=4),
    "T3sr": dict(dim=3, wraps=(1, 0, 2), periods=(4.0, 4.0, 8.0), span=4.0, n=2500, nq=128, seed=4),
}
SEED = 7100


def sq(a, b):
    """squared distance over the last axis, accumulated left to right (orc_euclid, sq3 / sq4 of the device)"""
    t = a[..., 0] - b[..., 0]
    s = t * t
    for i in range(1, a.shape[-1]):
        t = a[..., i] - b[..., i]
        s = s + t * t
    return s


def copies(Q, wraps, periods):
    """(ghost, closest) of every copy: two arrays (2^w, nq, dim); copy 0 is the query itself"""
    Q = np.asarray(Q, dtype=np.float64)
    w = len(wraps)
    G = np.repeat(Q[None], 1 << w, axis=0)
    Cl = G.copy()
    for k in range(1 << w):
        for n, (dim, per) in enumerate(zip(wraps, periods)):
            if not (k >> (w - 1 - n)) & 1:
                continue
            low = Q[:, dim] < per / 2.0
            G[k, :, dim] = np.where(low, Q[:, dim] + per, Q[:, dim] - per)
            Cl[k, :, dim] = np.where(low, per, 0.0)
    return G, Cl


def searched(Q, r, wraps, periods):
    """(2^w, nq) bool: which copies getNextGhostPoint hands out for range r (scalar or one per query)"""
    G, Cl = copies(Q, wraps, periods)
    v = ~(np.sqrt(sq(Cl, G)) > np.asarray(r, dtype=np.float64))
    v[0] = True
    return v


def reach(nodes, Q, r, wraps, periods):
    """dist (2^w, nq, n): sqrt(sq(copy, node)); hit (2^w, nq, n): copy is searched and lists the node by its own rule"""
    nodes = np.asarray(nodes, dtype=np.float64)
    G, _ = copies(Q, wraps, periods)
    rr = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(G[0]),))[None, :, None]
    dist = np.sqrt(sq(G[:, :, None, :], nodes[None, None, :, :]))
    hit = (dist < rr) & searched(Q, r, wraps, periods)[:, :, None]
    hit[0, :, 0] = dist[0, :, 0] <= rr[0, :, 0]                       # the root's <=, copy 0 alone
    return dist, hit


def range_lists(nodes, Q, r, wraps, periods):
    """kdFindWithinRange of every query as a CSR in ascending node index: dict(offsets, idx, key, slot)"""
    dist, hit = reach(nodes, Q, r, wraps, periods)
    listed = hit.any(axis=0)
    first = hit.argmax(axis=0)                                         # the first copy that lists the node
    qi, ni = np.nonzero(listed)                                        # row-major: queries in order, nodes ascending
    offsets = np.zeros(len(Q) + 1, dtype=np.int64)
    np.cumsum(listed.sum(axis=1), out=offsets[1:])
    slot = first[qi, ni]
    return dict(offsets=offsets, idx=ni.astype(np.int32), key=dist[slot, qi, ni], slot=slot)


def nearest(nodes, Q, wraps, periods):
    """kdFindNearest's distance per query: the query's own minimum, then every ghost that the iterator hands out for
    the best distance so far, each taken when strictly smaller"""
    nodes = np.asarray(nodes, dtype=np.float64)
    G, Cl = copies(Q, wraps, periods)
    best = np.sqrt(sq(G[0][:, None, :], nodes[None])).min(axis=1)
    skip = np.sqrt(sq(Cl, G))
    for k in range(1, len(G)):
        go = ~(skip[k] > best)
        d = np.sqrt(sq(G[k][:, None, :], nodes[None])).min(axis=1)
        best = np.where(go & (d < best), d, best)
    return best


def copy_dists(points, Q, wraps, periods):
    """(2^w, nq): distance of every copy of query i to points[i] (the check of a nearest index on a lattice of ties)"""
    G, _ = copies(Q, wraps, periods)
    return np.sqrt(sq(G, np.asarray(points, dtype=np.float64)[None]))


def cases(nodes, Q, r, wraps, periods):
    """The boundary cases of one scene at one radius (scalar or per query), counted on the restatement alone"""
    Q = np.asarray(Q, dtype=np.float64)
    rq = np.broadcast_to(np.asarray(r, dtype=np.float64), (len(Q),))
    G, Cl = copies(Q, wraps, periods)
    v = searched(Q, r, wraps, periods)
    dist, hit = reach(nodes, Q, r, wraps, periods)
    listed = hit.any(axis=0)
    at_r = (dist == rq[None, :, None]) & v[:, :, None]
    seen = hit.sum(axis=0)
    first = hit.argmax(axis=0)
    key = np.take_along_axis(dist, first[None], axis=0)[0]
    dmin = np.where(v[:, :, None], dist, np.inf).min(axis=0)
    wq = Q[:, list(wraps)]
    per = np.asarray(periods)
    return dict(
        all_copies=int(v.all(axis=0).sum()),
        on_skip=int((np.sqrt(sq(Cl, G))[1:] == rq[None]).sum()),
        at_r_unlisted=int((at_r.any(axis=0) & ~listed).sum()),
        multi_seen=int((seen >= 2).sum()),
        key_not_min=int((listed & (key != dmin)).sum()),
        at_half=int((wq == per / 2.0).any(axis=1).sum()),
        at_zero=int((wq == 0.0).any(axis=1).sum()),
        at_period=int((wq == per).any(axis=1).sum()),
        root_at_r_listed=int((dist[0, :, 0] == rq).sum()),
        root_at_r_ghost=int((at_r[1:, :, 0].any(axis=0) & ~listed[:, 0]).sum()),
        # the root exactly at r from a searched ghost (which does not list it) and listed by a LATER copy: the root's
        # <= must not leak into "an earlier copy has seen it"
        root_at_r_then_later=int((listed[:, 0] & (at_r[:, :, 0] & (np.arange(len(v))[:, None] >= 1)
                                                   & (np.arange(len(v))[:, None] < first[None, :, 0])).any(axis=0)).sum()),
        neighbours=int(listed.sum()),
    )


def _axis(rng, n, top, seam):
    """n multiples of 1/4 in [0, top]; seam: a third of them within 1.5 of an end, a tenth on 0, top / 2 or top"""
    q = rng.integers(0, int(4 * top) + 1, n)
    if seam:
        u = rng.uniform(size=n)
        near = rng.integers(0, 7, n)
        near = np.where(rng.uniform(size=n) < 0.5, near, int(4 * top) - near)
        q = np.where(u < 0.35, near, q)
        q = np.where(u > 0.9, rng.choice([0, int(2 * top), int(4 * top)], n), q)
    return q / 4.0


def _draw(sp, rng, n, seam):
    P = np.zeros((n, sp["dim"]))
    for d in range(sp["dim"]):
        if d in sp["wraps"]:
            per = sp["periods"][sp["wraps"].index(d)]
            if per == TWO_PI:
                P[:, d] = rng.integers(0, 9, n) * (math.pi / 4)        # 0 and 2 pi, the wrap point itself, included
            else:
                P[:, d] = _axis(rng, n, per, seam)
        else:
            P[:, d] = _axis(rng, n, sp["span"], False)
    return P


def _plant(sp, nodes, Q, radii):
    """Move two queries per radius onto the root's boundary cases: query i of radius i has the root exactly at r from
    itself (listed, <=); query len(radii) + i has it exactly at r from a searched ghost and inside no copy (not
    listed); query 2 len(radii) + i has it exactly at r from a searched ghost and listed by a later copy alone (only
    where two short periods meet).  The candidates are the lattice points of the space itself (theta of D4 left at the root's); the first
    in lexicographic order that qualifies is taken.  A radius with no such point in the space keeps its query."""
    axes = []
    for d in range(sp["dim"]):
        if d in sp["wraps"]:
            per = sp["periods"][sp["wraps"].index(d)]
            axes.append(nodes[:1, d] if per == TWO_PI else np.arange(0, int(4 * per) + 1) / 4.0)
        else:
            axes.append(np.arange(0, int(4 * sp["span"]) + 1) / 4.0)
    cand = np.stack([a.ravel() for a in np.meshgrid(*axes, indexing="ij")], axis=1)
    for i, r in enumerate(radii):
        G, Cl = copies(cand, sp["wraps"], sp["periods"])
        v = searched(cand, r, sp["wraps"], sp["periods"])
        dist = np.sqrt(sq(G, nodes[0][None, None, :]))
        own = dist[0] == r
        inside = ((dist < r) & v).any(axis=0) | (dist[0] <= r)
        ghost = ((dist[1:] == r) & v[1:]).any(axis=0) & ~inside
        if own.any():
            Q[i] = cand[np.argmax(own)]
        if ghost.any():
            Q[len(radii) + i] = cand[np.argmax(ghost)]
        hit = (dist < r) & v
        hit[0] = dist[0] <= r
        first = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
        k = np.arange(len(v))[:, None]
        later = ((dist == r) & v & (k >= 1) & (k < first[None])).any(axis=0)
        if later.any():
            Q[2 * len(radii) + i] = cand[np.argmax(later)]


def _plant_on_skip(sp, Q, r_mix, count):
    """Put `count` queries, taken from the end of the batch, exactly on the skip threshold of their own radius in the
    first wrapped lattice dimension whose period allows it: coordinate r (the ghost goes up and is r from the period)
    and period - r (it goes down and is r from 0) in turn.  Only radii r < period / 2 can sit there."""
    done = 0
    for i in range(len(Q) - 1, 3 * len(RADII) - 1, -1):
        if done >= count:
            break
        for d, per in zip(sp["wraps"], sp["periods"]):
            r = r_mix[i]
            if per != TWO_PI and r < per / 2.0:
                Q[i, d] = r if done % 2 == 0 else per - r
                done += 1
                break


def build(sp, rng, name="drawn"):
    """a scene of the space sp = dict(dim, wraps, periods, span, n, nq): distinct lattice nodes in a random order,
    queries drawn towards the seams, the root cases planted, the radii and the per-query array that mixes them"""
    nodes = np.unique(_draw(sp, rng, sp["n"], False), axis=0)
    nodes = nodes[rng.permutation(len(nodes))]
    Q = _draw(sp, rng, sp["nq"], True)
    _plant(sp, nodes, Q, RADII)
    r_mix = np.array([RADII[i % len(RADII)] for i in range(len(Q))])   # query i of _plant keeps its own radius
    _plant_on_skip(sp, Q, r_mix, sp.get("on_skip", 0))
    for a in (nodes, Q, r_mix):
        a.setflags(write=False)
    return dict(name=name, dim=sp["dim"], wraps=tuple(sp["wraps"]), periods=tuple(sp["periods"]), nodes=nodes, Q=Q,
                radii=RADII, r_mix=r_mix)


@functools.lru_cache(maxsize=None)
def _scene(name, seed):
    sp = SPACES[name]
    return build(sp, np.random.default_rng(SEED + 16 * sp["seed"] + seed), name)


def scene(name, seed=0):
    """dict(name, dim, wraps, periods, nodes, Q, radii, r_mix) of a space of SPACES, built once per session; the arrays
    are read-only.  r_mix is the per-query radius array that mixes the radii."""
    return _scene(name, seed)


# ---- nodes below 0 in a wrapped dimension ---------------------------------------------------------------------------
# With every node inside [0, period] two of the rules decide nothing: a query at exactly period / 2 is never farther
# from a node than either of its shifted copies, whichever side the copy goes to, and a ghost exactly on the skip
# threshold has its nearest possible node exactly at r.  The reference does not confine nodes to the period.  In this
# scene (T3's space) every node lies 1/4 .. 1 BELOW 0 in the first dimension, half of the queries have x = period / 2
# (the strict < sends their ghost to x - period, 3 .. 3.75 from the nodes; <= would send it to x + period) and half
# have x = period - r for a radius r (the ghost of the first dimension sits exactly on the skip threshold and is the
# only copy that reaches the nodes next to it).
SIDE = dict(dim=3, wraps=(0, 1, 2), periods=(8.0, 4.0, 8.0))


@functools.lru_cache(maxsize=None)
def side_scene(axis=0):
    """axis 0 (period 8): as described above.  axis 1 (period 4): the nodes lie below 0 in y and every query has
    y = 2 = period / 2, whose ghost is searched from r = 2.5 on (skip distance 2): the side test decides range lists too."""
    rng = np.random.default_rng(SEED + 900 + axis)
    n, nq = 200, 64
    # the other coordinates stay in the middle of their periods: a copy shifted there is never the nearer one, so
    # kdFindNearest is still the minimum over all copies (its skip rule presumes nodes inside the period)
    mid = {0: (14, 19), 1: (7, 10), 2: (14, 19)}
    nodes = np.stack([-rng.integers(1, 5, n) / 4.0 if d == axis else rng.integers(*mid[d], n) / 4.0 for d in range(3)], axis=1)
    nodes = np.unique(nodes, axis=0)
    nodes = nodes[rng.permutation(len(nodes))]
    half = SIDE["periods"][axis] / 2.0
    Q = np.stack([np.full(nq, half) if d == axis else rng.integers(*mid[d], nq) / 4.0 for d in range(3)], axis=1)
    r_mix = np.array([RADII[i % len(RADII)] for i in range(nq)])
    if axis == 0:
        odd = np.arange(nq) % 8 >= 4
        Q[odd, 0] = 8.0 - r_mix[odd]
    for a in (nodes, Q, r_mix):
        a.setflags(write=False)
    return dict(name=f"side{axis}", nodes=nodes, Q=Q, radii=RADII, r_mix=r_mix, **SIDE)


# ---- a planar torus for the obstacle sweeps ---------------------------------------------------------------------------
SWEEP_RR, SWEEP_DELTA = 0.25, 1.0                     # robot radius + delta = 1.25; + a half diagonal of 1.25 / 2.5
HALF_SIDES = ((0.75, 1.0), (1.0, 0.75), (1.5, 2.0))   # half diagonals 1.25, 1.25, 2.5: ranges 2.5, 2.5, 3.75
PLANE = dict(dim=3, wraps=(0, 1), periods=(8.0, 4.0))


def planar_scene(seed=0, m=10):
    """dim 3 at z = 0, x and y wrapped with periods 8 and 4: distinct lattice nodes, m lattice boxes and right triangles
    whose bounding-box centre is a lattice point (the first four next to the four corners of the period, where the
    copy that shifts both dimensions is the only one to reach the nodes of the opposite corner) and whose search
    range (robot radius + delta + half diagonal) is a lattice distance, and a mirror of three out-edges per node: to
    the next node, to a random one and to the node nearest the centre of one obstacle (an edge that ends inside it).
    dict(nodes, polys, centres, ranges, es, ee) + PLANE."""
    rng = np.random.default_rng(SEED + 500 + seed)
    xy = np.unique(np.stack([rng.integers(0, 33, 450) / 4.0, rng.integers(0, 17, 450) / 4.0], axis=1), axis=0)
    xy = xy[rng.permutation(len(xy))]
    nodes = np.c_[xy, np.zeros(len(xy))]
    n = len(nodes)
    centres = np.stack([rng.integers(4, 29, m) / 4.0, rng.integers(2, 15, m) / 4.0], axis=1)
    centres[:4] = [[0.5, 0.5], [7.5, 3.5], [0.25, 3.75], [7.75, 0.25]]
    polys, ranges = [], []
    for j in range(m):
        a, b = HALF_SIDES[j % len(HALF_SIDES)]
        c = centres[j]
        if j % 2 == 0:
            v = [[-a, -b], [a, -b], [a, b], [-a, b]]                  # box
        else:
            v = [[-a, -b], [a, -b], [-a, b]]                          # right triangle: the same bounding box and radius
        polys.append(c + np.array(v))
        ranges.append(SWEEP_RR + SWEEP_DELTA + math.sqrt(a * a + b * b))
    near = [int(np.argmin(sq(nodes[:, :2], c[None]))) for c in centres]
    i = np.arange(n)
    es = np.concatenate([i, i, i]).astype(np.int32)
    ee = np.concatenate([(i + 1) % n, rng.integers(0, n, n), np.array(near)[i % m]]).astype(np.int32)
    return dict(nodes=nodes, polys=polys, centres=centres, ranges=np.array(ranges), es=es, ee=ee, **PLANE)
