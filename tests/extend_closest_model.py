"""The reference for rrtx_extend_closest_self (the k nearest earlier samples of an extend batch, for the closestNode
rule), from numpy and the oracle alone: all pairs (s, i) with the unfused fp64 sq3, sorted per row, and
oracle.edges_check_batch over the whole obstacle list for the flags.  The scenes are those of tests/extend_self_model.py.
tests/test_extend_closest_scenes.py holds the model to the oracle's kdFindNearest and the scenes to the cases they are
there for; the GPU tests compare against it bit for bit."""
import functools

import numpy as np

import extend_self_model as S

RR = S.RR
MAX_K = 32
FIELDS = ("idx", "cost", "hit_out", "hit_in", "count")
TREE_FIELDS = ("tree_hit_out", "tree_hit_in")
# a marked sample and a non-finite one in the middle of a batch (positions in the "mid" scene)
MARKED, NOT_FINITE = 100, 131


def sq3_all(Q):
    """s[j, i] = sq3(q_j, q_i), the expression of the self join: ((dx * dx) + (dy * dy)) + (dz * dz), nothing fused"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = Q[:, None, :] - Q[None, :, :]
        s = d[..., 0] * d[..., 0]
        s = s + d[..., 1] * d[..., 1]
        s = s + d[..., 2] * d[..., 2]
    return s


def live_samples(Q, skip=None):
    live = np.isfinite(Q).all(axis=1)
    if skip is not None:
        live &= np.asarray(skip).reshape(-1) == 0
    return live


def ranked_rows(Q, skip=None):
    """per sample j the live samples i < j with finite s, ordered by (s, i): a list of (i, s) array pairs"""
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    s, live = sq3_all(Q), live_samples(Q, skip)
    rows = []
    for j in range(len(Q)):
        i = np.flatnonzero(live[:j] & np.isfinite(s[j, :j]))
        o = np.lexsort((i, s[j, i]))
        rows.append((i[o], s[j, i[o]]))
    return rows


def closest_reference(oracle, Q, k, obs, robot_radius=RR, skip=None, want=None, tree_idx=None, tree_pts=None):
    """What rrtx_extend_closest_self returns: dict(idx, cost, hit_out, hit_in: (nq, k); count: (nq,); tree_hit_out,
    tree_hit_in: (nq,) when tree_idx is given)"""
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    nq = len(Q)
    filled = live_samples(Q, skip)
    if want is not None:
        filled &= np.asarray(want).reshape(-1) != 0
    out = dict(idx=np.full((nq, k), -1, dtype=np.int32), cost=np.full((nq, k), np.inf),
               hit_out=np.zeros((nq, k), dtype=np.uint8), hit_in=np.zeros((nq, k), dtype=np.uint8),
               count=np.zeros(nq, dtype=np.int32))
    rows = ranked_rows(Q, skip)
    for j in np.flatnonzero(filled):
        i, s = rows[j]
        n = min(k, len(i))
        out["idx"][j, :n] = i[:n]
        out["cost"][j, :n] = np.sqrt(s[:n])
        out["count"][j] = n
    jj, slot = np.nonzero(out["idx"] >= 0)
    if len(jj):
        ii = out["idx"][jj, slot]
        out["hit_out"][jj, slot] = oracle.edges_check_batch(obs, Q[jj], Q[ii], robot_radius)[0]
        out["hit_in"][jj, slot] = oracle.edges_check_batch(obs, Q[ii], Q[jj], robot_radius)[0]
    if tree_idx is not None:
        tree_idx = np.asarray(tree_idx).reshape(-1)
        n_tree = 0 if tree_pts is None else len(tree_pts)
        out["tree_hit_out"], out["tree_hit_in"] = np.zeros(nq, dtype=np.uint8), np.zeros(nq, dtype=np.uint8)
        jj = np.flatnonzero(filled & (tree_idx >= 0) & (tree_idx < n_tree))
        if len(jj):
            P = np.ascontiguousarray(tree_pts, dtype=np.float64)[tree_idx[jj]]
            out["tree_hit_out"][jj] = oracle.edges_check_batch(obs, Q[jj], P, robot_radius)[0]
            out["tree_hit_in"][jj] = oracle.edges_check_batch(obs, P, Q[jj], robot_radius)[0]
    return out


def narrow(ref, b, k):
    """the result for the first b samples and k slots, from one for more of both: a row depends on the samples before
    it alone, and the first k of a longer row are the row"""
    out = {f: ref[f][:b, :k].copy() for f in FIELDS if f != "count"}
    out["count"] = np.minimum(ref["count"][:b], k).astype(np.int32)
    return out


def samples(name):
    return S.lattice_samples() if name == "lattice" else S.random_samples(name)


def marked_samples():
    """the "mid" batch with a non-finite sample and a marked one in the middle: (samples, skip)"""
    Q = S.random_samples("mid").copy()
    Q[NOT_FINITE, 1] = np.nan
    skip = np.zeros(len(Q), dtype=np.uint8)
    skip[MARKED] = 1
    return Q, skip


@functools.lru_cache(maxsize=None)
def scene(kind, name):
    """(samples, reference with MAX_K slots) of a scene, computed once per session; name: a key of S.RANDOM or
    "lattice" (spheres)"""
    from oracle import oracle
    oracle.lib()
    Q = samples(name)
    return Q, closest_reference(oracle, Q, MAX_K, S.obstacles(oracle, kind, name))
