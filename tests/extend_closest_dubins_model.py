"""The reference for rrtx_extend_closest_self_dubins (the k nearest earlier samples of a Dubins extend batch in the
wrapped space, for the closestNode rule), from numpy and the oracle alone: all pairs s(j, i) = the minimum over every
copy of q_j (tests/torus_model.py's rule for the copies, none skipped) of the unfused fp64 sq4 to q_i, a lexsort by
(s, i) per row, oracle.dubins_candidates_batch with the samples as the node table for costs and flags and
oracle.dubins_edges_batch for the words.  The scenes are those of tests/extend_self_dubins_model.py and one with three
wrapped dimensions.  tests/test_extend_closest_dubins_scenes.py holds the model to the oracle's kdFindNearest and the
scenes to the cases they are there for; the GPU tests compare against it bit for bit."""
import functools

import numpy as np

import extend_self_dubins_model as S
import torus_model

RR, RMIN = S.RR, S.RMIN
MAX_K = 32
ROW_FIELDS = ("idx", "key", "cost_out", "cost_in", "word_out", "word_in", "hit_out", "hit_in")
FIELDS = ROW_FIELDS + ("count",)
TREE_FIELDS = ("tree_cost_out", "tree_cost_in", "tree_word_out", "tree_word_in", "tree_hit_out", "tree_hit_in")
# a marked sample and a non-finite one in the middle of a batch (positions in the "mid" scene)
MARKED, NOT_FINITE = 100, 131
# x, t and theta wrapped: eight copies of a sample
THREE_WRAPS = ((0, 2, 3), (12.0, 4.0, S.TWO_PI))
NO_WORD = np.zeros(1, dtype="S3")[0]


def three_wrap_samples():
    """the two-wrap scene moved into [0, 12] in x, which is wrapped as well"""
    q = S.two_wrap_samples().copy()
    q[:, 0] += 6.0
    return q


def scene_inputs(name, mode="flat"):
    """(samples, (polygons, kinds, paths), wraps) of a scene; name: as in extend_self_dubins_model.scene_inputs, or
    "three" (the polygons of "mid" moved with the samples)"""
    if name == "three":
        polys, kinds, paths = S.polygon_args("mid", mode)
        assert paths is None
        return three_wrap_samples(), ([p + np.array([6.0, 0.0]) for p in polys], kinds, None), THREE_WRAPS
    Q, _, pa, wraps = S.scene_inputs(name, mode)
    return Q, pa, wraps


def sq4(a, c):
    """((dx * dx + dy * dy) + dz * dz) + dw * dw, nothing fused"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = a - c
        s = d[..., 0] * d[..., 0]
        s = s + d[..., 1] * d[..., 1]
        s = s + d[..., 2] * d[..., 2]
        return s + d[..., 3] * d[..., 3]


def s_all(Q, wraps):
    """(s[j, i], slot[j, i]): the minimum over all 2^w copies of q_j of sq4(copy, q_i), and the lowest slot attaining it"""
    G, _ = torus_model.copies(Q, list(wraps[0]), list(wraps[1]))
    with np.errstate(invalid="ignore"):
        per = np.stack([sq4(g[:, None, :], Q[None, :, :]) for g in G])
        per = np.where(np.isnan(per), np.inf, per)         # (a non-finite sample: it is in no row anyway)
    return per.min(axis=0), per.argmin(axis=0)


def live_samples(Q, skip=None):
    live = np.isfinite(Q).all(axis=1)
    if skip is not None:
        live &= np.asarray(skip).reshape(-1) == 0
    return live


def ranked_rows(Q, wraps=S.THETA, skip=None):
    """per sample j the live samples i < j with finite s, ordered by (s, i): a list of (i, s, slot) array triples"""
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 4)
    (s, slot), live = s_all(Q, wraps), live_samples(Q, skip)
    rows = []
    for j in range(len(Q)):
        i = np.flatnonzero(live[:j] & np.isfinite(s[j, :j]))
        o = np.lexsort((i, s[j, i]))
        rows.append((i[o], s[j, i[o]], slot[j, i[o]]))
    return rows


def _edges(oracle, Q, jj, nodes, ii, ps, mode):
    """both directed Dubins edges Q[jj] <-> nodes[ii]: (cost_out, cost_in, word_out, word_in, hit_out, hit_in)"""
    opt = S.MODES[mode]
    offsets = np.zeros(len(Q) + 1, dtype=np.int64)
    np.cumsum(np.bincount(jj, minlength=len(Q)), out=offsets[1:])
    assert (np.diff(jj) >= 0).all()
    c = oracle.dubins_candidates_batch(Q, offsets, ii.astype(np.int32), nodes, RMIN, ps, RR, **opt)
    eo = oracle.dubins_edges_batch(Q[jj], nodes[ii], RMIN, has_time=opt["has_time"], piecewise=opt["piecewise"])
    ei = oracle.dubins_edges_batch(nodes[ii], Q[jj], RMIN, has_time=opt["has_time"], piecewise=opt["piecewise"])
    assert np.array_equal(eo["cost"], c["cost_out"]) and np.array_equal(ei["cost"], c["cost_in"])
    return c["cost_out"], c["cost_in"], eo["word"], ei["word"], c["hit_out"], c["hit_in"]


def closest_reference(oracle, Q, k, ps, mode="flat", wraps=S.THETA, skip=None, want=None, tree_idx=None, tree_pts=None):
    """What rrtx_extend_closest_self_dubins returns: dict(idx, key, cost_out, cost_in, word_out, word_in, hit_out,
    hit_in: (nq, k); count: (nq,); the six tree_* fields: (nq,) when tree_idx is given)"""
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 4)
    nq = len(Q)
    filled = live_samples(Q, skip)
    if want is not None:
        filled &= np.asarray(want).reshape(-1) != 0
    out = dict(idx=np.full((nq, k), -1, dtype=np.int32), key=np.full((nq, k), np.inf), cost_out=np.full((nq, k), np.inf),
               cost_in=np.full((nq, k), np.inf), word_out=np.zeros((nq, k), dtype="S3"), word_in=np.zeros((nq, k), dtype="S3"),
               hit_out=np.zeros((nq, k), dtype=np.uint8), hit_in=np.zeros((nq, k), dtype=np.uint8),
               count=np.zeros(nq, dtype=np.int32))
    rows = ranked_rows(Q, wraps, skip)
    for j in np.flatnonzero(filled):
        i, s, _ = rows[j]
        n = min(k, len(i))
        out["idx"][j, :n] = i[:n]
        out["key"][j, :n] = np.sqrt(s[:n])
        out["count"][j] = n
    jj, slot = np.nonzero(out["idx"] >= 0)
    if len(jj):
        ii = out["idx"][jj, slot]
        vals = _edges(oracle, Q, jj, np.where(np.isfinite(Q), Q, 0.0), ii, ps, mode)
        for f, v in zip(ROW_FIELDS[2:], vals):
            out[f][jj, slot] = v
    if tree_idx is not None:
        tree_idx = np.asarray(tree_idx).reshape(-1)
        n_tree = 0 if tree_pts is None else len(tree_pts)
        out.update(tree_cost_out=np.full(nq, np.inf), tree_cost_in=np.full(nq, np.inf),
                   tree_word_out=np.zeros(nq, dtype="S3"), tree_word_in=np.zeros(nq, dtype="S3"),
                   tree_hit_out=np.zeros(nq, dtype=np.uint8), tree_hit_in=np.zeros(nq, dtype=np.uint8))
        jj = np.flatnonzero(filled & (tree_idx >= 0) & (tree_idx < n_tree))
        if len(jj):
            vals = _edges(oracle, Q, jj, np.ascontiguousarray(tree_pts, dtype=np.float64), tree_idx[jj], ps, mode)
            for f, v in zip(TREE_FIELDS, vals):
                out[f][jj] = v
    return out


def narrow(ref, b, k):
    """the result for the first b samples and k slots, from one for more of both: a row depends on the samples before
    it alone, and the first k of a longer row are the row"""
    out = {f: ref[f][:b, :k].copy() for f in ROW_FIELDS}
    out["count"] = np.minimum(ref["count"][:b], k).astype(np.int32)
    return out


def marked_samples():
    """the "mid" batch with a non-finite sample and a marked one in the middle: (samples, skip)"""
    Q = S.random_samples("mid").copy()
    Q[NOT_FINITE, 1] = np.nan
    skip = np.zeros(len(Q), dtype=np.uint8)
    skip[MARKED] = 1
    return Q, skip


def polygon_set(oracle, name, mode="flat"):
    _, (polys, kinds, paths), _ = scene_inputs(name, mode)
    return oracle.PolygonSet(polys, kinds=kinds, paths=paths)


@functools.lru_cache(maxsize=None)
def scene(name, mode="flat"):
    """(samples, reference with MAX_K slots, wraps) of a scene, computed once per session"""
    from oracle import oracle
    oracle.lib()
    Q, _, wraps = scene_inputs(name, mode)
    return Q, closest_reference(oracle, Q, MAX_K, polygon_set(oracle, name, mode), mode, wraps), wraps
