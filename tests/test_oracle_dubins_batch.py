"""The batched Dubins entry points of the oracle (orc_dubins_edges_batch, orc_dubins_candidates_batch) against the
per-edge wrappers they loop over: bit for bit, with and without time, both time columns, on random edges, the
lattice poses of tests/test_gpu_parity.py::test_dubins_degenerate_poses_exact and the longest polylines steering
can produce.  CPU only: the dense GPU tests (tests/test_gpu_dubins_dense.py) trust the batch form because of this."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import synth

RR = 0.5
ARC_ROWS = int(math.ceil(2.0 * math.pi / 0.1)) + 1        # rows of one full turn at delta_phi = 0.1 (:506)


def _lattice():
    hd = np.arange(8) * (math.pi / 4)
    s_l, g_l = [], []
    for ti in hd:
        for tg in hd:
            for dx in (-4.0, -2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 8.0):
                for dy in (-4.0, -2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 4.0):
                    s_l.append([1.0, -2.0, 20.0, ti]); g_l.append([1.0 + dx, -2.0 + dy, 18.5, tg])
    return np.array(s_l), np.array(g_l)


def _edges(has_time: bool):
    """random edges over the synth world, lattice poses (every 3rd), goals just behind the start with about its
    heading (long turns on both sides) and far goals"""
    rng = np.random.default_rng(41)
    n = 2400
    s = synth.nodes(n, 4, seed=synth.SEED + 31)
    g = s.copy()
    g[:, :2] += rng.normal(0.0, 6.0, (n, 2))
    g[:, 3] = rng.uniform(0.0, 2.0 * math.pi, n)
    ls, lg = _lattice()
    ls, lg = ls[::3], lg[::3]
    k = 200
    ts = np.zeros((k, 4)); tg = np.zeros((k, 4))
    ts[:, :2] = rng.uniform(-40, 40, (k, 2)); ts[:, 3] = rng.uniform(0, 2 * math.pi, k)
    back = rng.uniform(0.0, 0.3, k)
    tg[:, 0] = ts[:, 0] - back * np.cos(ts[:, 3]); tg[:, 1] = ts[:, 1] - back * np.sin(ts[:, 3])
    tg[:, 3] = ts[:, 3] + rng.normal(0.0, 0.05, k)
    fs = synth.nodes(k, 4, seed=synth.SEED + 32); fg = synth.nodes(k, 4, seed=synth.SEED + 33)
    fg[:, :2] *= 40.0                                            # goals up to 2000 away
    S = np.concatenate([s, ls, ts, fs]); G = np.concatenate([g, lg, tg, fg])
    if has_time:
        t0 = rng.uniform(synth.T_MIN, synth.T_MAX, len(S))
        S[:, 2] = t0
        G[:, 2] = t0 - rng.uniform(0.05, 4.0, len(S))
        G[::9, 2] = t0[::9] + rng.uniform(0.0, 1.0, len(S[::9]))       # some the wrong way in time (validMove false)
        S[len(s):len(s) + len(ls), 2] = 20.0; G[len(s):len(s) + len(ls), 2] = 18.5
    return S, G


def _per_edge(oracle, ps, s, g, r_min, has_time, piecewise):
    if has_time:
        d, w, v, wd, tr = oracle.dubins_steer_time(s, g, r_min, piecewise=piecewise)
        h, fh = oracle.dubins_edge_check_polygons_time(ps, s, g, tr, RR, r_min)
        ok = oracle.dubins_valid_move_time(s, g, v, synth.V_MIN, synth.V_MAX)
        return d, w, v, wd, tr, h, fh, ok
    c, wd, tr = oracle.dubins_steer(s, g, r_min)
    h, fh = oracle.dubins_edge_check_polygons(ps, s, g, tr, RR, r_min)
    return c, c, float("nan"), wd, tr, h, fh, True


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("has_time,piecewise", [(False, False), (True, False), (True, True)])
def test_edges_batch_equals_per_edge(oracle, has_time, piecewise):
    S, G = _edges(has_time)
    if has_time:
        polys, kinds, paths, active, _ = synth.dynamic_polygons(48)
        ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=active)
    else:
        ps = oracle.PolygonSet(synth.polygons(48))
    compared = 0
    words, hits = set(), 0
    for r_min in (1.0, 2.0):
        out = oracle.dubins_edges_batch(S, G, r_min, ps, RR, has_time=has_time, piecewise=piecewise,
                                        v_min=synth.V_MIN, v_max=synth.V_MAX, traj=True, threads=3)
        off, rows = out["traj_off"], out["traj"]
        assert rows.shape[1] == (3 if has_time else 2)
        for i in range(len(S)):
            d, w, v, wd, tr, h, fh, ok = _per_edge(oracle, ps, S[i], G[i], r_min, has_time, piecewise)
            assert _same(out["cost"][i], d) and _same(out["wdist"][i], w) and _same(out["velocity"][i], v), i
            assert out["word"][i].decode() == wd and out["traj_len"][i] == len(tr), i
            assert bool(out["hit"][i]) == h and out["first_hit"][i] == fh and bool(out["valid_move"][i]) == ok, i
            assert _same(rows[off[i]:off[i + 1]], tr), i
            words.add(wd); hits += h
        compared += len(S)
        # the per-edge wrappers hold 1024 rows: no edge comes near that (three arcs of at most a full turn each; the
        # longest found in 400 k random short edges have 94 rows).  Edges past one full turn's rows are in the set,
        # so the batch's trajectory scratch (64 rows at first) grew on them.
        assert out["traj_len"].max() <= 3 * ARC_ROWS < 1024
        assert out["traj_len"].max() > ARC_ROWS + 20
    assert compared >= 2000 * 2
    assert {"lsl", "rsr", "lsr", "rsl", "rlr", "lrl"} <= words
    assert 0 < hits < compared
    if has_time:
        assert 0 < out["valid_move"].mean() < 1


def test_edges_batch_traj_subset_and_threads(oracle):
    S, G = _edges(True)
    mask = np.zeros(len(S), dtype=bool); mask[::7] = True
    a = oracle.dubins_edges_batch(S, G, 2.0, has_time=True, piecewise=True, traj=mask, threads=1)
    b = oracle.dubins_edges_batch(S, G, 2.0, has_time=True, piecewise=True, traj=True, threads=16)
    for k in ("cost", "wdist", "velocity", "traj_len", "valid_move"):
        assert _same(a[k], b[k]), k
    assert np.array_equal(a["word"], b["word"])
    assert np.array_equal(np.diff(a["traj_off"]), np.where(mask, a["traj_len"], 0))
    for i in np.flatnonzero(mask):
        assert _same(a["traj"][a["traj_off"][i]:a["traj_off"][i + 1]], b["traj"][b["traj_off"][i]:b["traj_off"][i + 1]])


def test_edges_batch_moving_obstacles_need_time(oracle):
    """the oracle has no branch for moving obstacles without time: an error, never a miss"""
    polys, kinds, paths, active, _ = synth.dynamic_polygons(16)
    ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=active)
    S, G = _edges(False)
    with pytest.raises(ValueError):
        oracle.dubins_edges_batch(S[:50], G[:50], 1.0, ps, RR)


@pytest.mark.parametrize("has_time", [False, True])
def test_candidates_batch_equals_edges_batch(oracle, has_time):
    rng = np.random.default_rng(5)
    nodes = synth.nodes_time(3000) if has_time else synth.nodes(3000, 4)
    Q = synth.nodes_time(40, seed=synth.SEED + 7) if has_time else synth.queries(40, 4)
    counts = rng.integers(0, 60, len(Q)); counts[[3, 17]] = 0           # samples without neighbours too
    off = np.zeros(len(Q) + 1, dtype=np.int64); np.cumsum(counts, out=off[1:])
    idx = rng.integers(0, len(nodes), int(off[-1])).astype(np.int32)
    if has_time:
        polys, kinds, paths, active, _ = synth.dynamic_polygons(32)
        ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=active)
    else:
        ps = oracle.PolygonSet(synth.polygons(32))
    r_min = synth.R_MIN_TIME if has_time else 1.0
    kw = dict(has_time=has_time, piecewise=True, v_min=synth.V_MIN, v_max=synth.V_MAX)
    cand = oracle.dubins_candidates_batch(Q, off, idx, nodes, r_min, ps, RR, threads=4, **kw)
    owner = np.repeat(np.arange(len(Q)), counts)
    for (a, b, sfx) in ((Q[owner], nodes[idx], "out"), (nodes[idx], Q[owner], "in")):
        e = oracle.dubins_edges_batch(a, b, r_min, ps, RR, **kw)
        flag = e["hit"] | np.where(has_time & (e["valid_move"] == 0), 2, 0).astype(np.uint8)
        assert _same(cand["cost_" + sfx], e["cost"]) and np.array_equal(cand["hit_" + sfx], flag), sfx
        assert np.array_equal(cand["traj_len_" + sfx], e["traj_len"]), sfx
    assert (cand["hit_out"] & 1).any()
    if has_time:
        assert ((cand["hit_out"] | cand["hit_in"]) & 2).any()
    else:
        assert not ((cand["hit_out"] | cand["hit_in"]) & 2).any()
