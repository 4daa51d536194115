"""Every Dubins edge of one C3 call and one C5 call against the oracle, not a sample.  The steering and check kernels
(dubins_steer_rec_kernel, dubins_check_rec_kernel<TIME>) run in chunks of 2^21 edges (kDubChunk,
rrtqx_3d_amd/csrc/kernels_dubins.hip), so each call here holds more than 2^21 CSR entries and the later chunks are
compared too.  The oracle side is the batched form of the per-edge functions (oracle.dubins_edges_batch /
dubins_candidates_batch, held equal to the per-edge wrappers by tests/test_oracle_dubins_batch.py).  Every comparison
is == on doubles and bytes; every test asserts how many directed edges it compared.  The CSR the preamble builds is
compared with the oracle's range search (oracle.range_batch) entry for entry first."""
import math

import numpy as np
import pytest

from rrtqx_3d_amd import synth
from rrtqx_3d_amd.context import Context

pytestmark = pytest.mark.gpu
RR = 0.5
CHUNK = 1 << 21                      # kDubChunk
WORDS = {b"lsl", b"rsr", b"lsr", b"rsl", b"rlr", b"lrl"}
C3_SAMPLES, C3_ENTRIES = 1600, 2_228_958          # CSR entries of the samples' range searches (the oracle's kd-tree)
C5_SAMPLES, C5_ENTRIES = 1024, 2_390_051
N_TRAJ = 100_000


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _trajectory_rows(oracle, ctx, s, g, tl, pool, words, r_min, has_time, seed):
    """dubins_trajectory, row for row, on N_TRAJ random edges of the set plus its longest polylines and edges of
    every word (from the edges `pool` whose `words` are known); returns (edges compared, longest polyline)"""
    rng = np.random.default_rng(seed)
    longest = np.argsort(tl, kind="stable")[-2000:]
    by_word = np.concatenate([pool[np.flatnonzero(words == w)[:200]] for w in sorted(WORDS)])
    sel = np.unique(np.concatenate([rng.choice(len(s), N_TRAJ, replace=False), longest, by_word]))
    off, rows = ctx.dubins_trajectory(s[sel], g[sel], r_min)
    ref = oracle.dubins_edges_batch(s[sel], g[sel], r_min, has_time=has_time, piecewise=True, traj=True)
    assert rows.shape[1] == (3 if has_time else 2)
    assert np.array_equal(off, ref["traj_off"])
    assert _same(rows, ref["traj"])
    assert set(ref["word"].tolist()) == WORDS
    assert int(np.diff(off).max()) == int(tl.max())          # the longest polyline of the whole set is among them
    return len(sel), int(np.diff(off).max())


def test_c3_every_dubins_edge(oracle):
    """C3 (N = 50k, 64 polygons, wrapped theta, r = 10, r_min = 1): the fused preamble on 1 600 samples, every entry
    in both directions; the same directed edges through dubins_edges_check in one call (the spread = 1 mapping of
    the check kernel); the launch over a capacity far above the entries; polylines row for row."""
    cfg = synth.CONFIGS["C3"]
    N, M = cfg.n_nodes, cfg.n_obstacles
    pts = synth.nodes(N, 4)
    Q = synth.queries(cfg.batch, 4)[:C3_SAMPLES]
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    assert r == 10.0
    r_min = 1.0
    polys = synth.polygons(M)
    ps = oracle.PolygonSet(polys)
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.polygons_set(polys)
        out = ctx.extend_candidates_dubins(Q, r, RR, r_min, cap=C3_ENTRIES)
        off, idx = out["offsets"], out["idx"]
        n = len(idx)
        assert n == C3_ENTRIES > CHUNK
        # the preamble's CSR is the oracle's range search, entry for entry (the checks below take it as given)
        trees = oracle.TreeSet(4, pts, wraps=[3], wrap_points=[2.0 * math.pi])
        rng = oracle.range_batch(trees, Q, r, per_sample=1500, nearest=False)
        del trees
        oracle.assert_same_results(out, rng, ("offsets", "idx", "key"), label="C3 Dubins preamble CSR: ")
        owner = np.repeat(np.arange(len(Q)), np.diff(off))
        s = np.concatenate([Q[owner], pts[idx]])                 # sample -> node, then node -> sample
        g = np.concatenate([pts[idx], Q[owner]])
        ref = oracle.dubins_edges_batch(s, g, r_min, ps, RR)
        # the fused preamble, every entry, both directions (no time: the flag byte is the collision bit alone)
        assert _same(out["cost_out"], ref["cost"][:n]) and _same(out["cost_in"], ref["cost"][n:])
        assert np.array_equal(out["hit_out"], ref["hit"][:n]) and np.array_equal(out["hit_in"], ref["hit"][n:])
        assert np.array_equal(out["word_out"], ref["word"][:n]) and np.array_equal(out["word_in"], ref["word"][n:])
        # the same 2n directed edges in one dubins_edges_check call
        cost, word, hit, tl = ctx.dubins_edges_check(s, g, r_min, RR)
        assert _same(cost, ref["cost"]) and np.array_equal(word, ref["word"])
        assert np.array_equal(hit, ref["hit"]) and np.array_equal(tl, ref["traj_len"])
        assert 0.01 < hit.mean() < 0.9 and set(word.tolist()) == WORDS
        # a capacity far above the entries: the launch covers cap, the outputs do not change
        out2 = ctx.extend_candidates_dubins(Q, r, RR, r_min, cap=2 * n + 4099)
        for k in ("offsets", "idx", "key", "cost_out", "cost_in", "word_out", "word_in", "hit_out", "hit_in"):
            assert np.array_equal(out2[k], out[k]), k
        n_traj, rows = _trajectory_rows(oracle, ctx, s, g, ref["traj_len"], np.arange(len(s)), ref["word"], r_min,
                                        False, 31)
    assert len(s) == 2 * C3_ENTRIES and n_traj >= N_TRAJ
    print(f"\nC3: {n} entries, {2 * n} directed edges (fused preamble and dubins_edges_check), "
          f"{n_traj} polylines row for row (longest {rows} rows)")


def test_c5_every_dubins_edge_with_time(oracle):
    """C5 with time (500k nodes, synth.dynamic_polygons(256) with its moving, inactive and hidden polygons,
    r = 7.1575, r_min = 2): the fused preamble on 1 024 samples in two obstacle states (active; active + hidden),
    every entry in both directions.  Costs and flag bytes equal the piecewise oracle (the time column as the kernels
    form it); the collision bit equals the reference's running-sum time column on every edge (zero flips).  Then
    dubins_steer_full on a slice and polylines row for row."""
    cfg = synth.CONFIGS["C5"]
    N, M = cfg.n_nodes, cfg.n_obstacles
    r = synth.ball_radius(N, 4, gamma=100.0, delta=10.0)
    assert abs(r - 7.1575) < 1e-3
    pts = synth.nodes_time(N)
    Q = synth.nodes_time(cfg.batch, seed=synth.SEED + 1)[:C5_SAMPLES]
    polys, kinds, paths, active, hidden = synth.dynamic_polygons(M)
    r_min = synth.R_MIN_TIME
    vel = dict(v_min=synth.V_MIN, v_max=synth.V_MAX)
    seen = active.copy()
    seen[hidden] = 1
    compared, flips, hits, first = 0, 0, [], None
    with Context(4, node_capacity=N) as ctx:
        ctx.set_wrap(3, 2.0 * math.pi)
        ctx.nodes_append(pts)
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(synth.V_MIN, synth.V_MAX)
        for act in (active, seen):
            ctx.polygons_set(polys, kinds=kinds, paths=paths, active=act)
            out = ctx.extend_candidates_dubins(Q, r, RR, r_min, cap=C5_ENTRIES)
            off, idx = out["offsets"], out["idx"]
            n = len(idx)
            assert n == C5_ENTRIES > CHUNK
            if first is None:                                # the preamble's CSR is the oracle's range search
                trees = oracle.TreeSet(4, pts, wraps=[3], wrap_points=[2.0 * math.pi])
                rng = oracle.range_batch(trees, Q, r, per_sample=2400, nearest=False)
                del trees
                oracle.assert_same_results(out, rng, ("offsets", "idx", "key"), label="C5 Dubins preamble CSR: ")
            first = out if first is None else first
            assert np.array_equal(idx, first["idx"]) and np.array_equal(out["cost_out"], first["cost_out"])
            ps = oracle.PolygonSet(polys, kinds=kinds, paths=paths, active=act)
            pw = oracle.dubins_candidates_batch(Q, off, idx, pts, r_min, ps, RR, has_time=True, piecewise=True, **vel)
            rs = oracle.dubins_candidates_batch(Q, off, idx, pts, r_min, ps, RR, has_time=True, piecewise=False, **vel)
            for d in ("out", "in"):
                assert _same(out["cost_" + d], pw["cost_" + d]), d
                assert np.array_equal(out["hit_" + d], pw["hit_" + d]), d
                assert _same(rs["cost_" + d], pw["cost_" + d]), d
                flips += int(np.count_nonzero((out["hit_" + d] & 1) != (rs["hit_" + d] & 1)))
            compared += 2 * n
            hits.append(int(np.count_nonzero(out["hit_out"] & 1)))
            assert (out["hit_out"] & 2).any() and (out["hit_out"] & 1).any()
        assert flips == 0                                       # the running-sum reference never decides otherwise
        assert hits[1] > hits[0]                                # the hidden polygons block more edges
        owner = np.repeat(np.arange(len(Q)), np.diff(off))
        s = np.concatenate([Q[owner], pts[idx]])
        g = np.concatenate([pts[idx], Q[owner]])
        tl = np.concatenate([pw["traj_len_out"], pw["traj_len_in"]])
        # calculateTrajectory's scalars on a slice of the same directed edges
        sl = np.random.default_rng(8).choice(len(s), 300_000, replace=False)
        full = ctx.dubins_steer_full(s[sl], g[sl], r_min)
        ref = oracle.dubins_edges_batch(s[sl], g[sl], r_min, has_time=True, piecewise=True, **vel)
        for k in ("dist", "wdist", "velocity"):
            assert _same(full[k], ref["cost" if k == "dist" else k]), k
        assert np.array_equal(full["word"], ref["word"]) and np.array_equal(full["valid_move"], ref["valid_move"])
        assert 0.05 < full["valid_move"].mean() < 0.95
        n_traj, rows = _trajectory_rows(oracle, ctx, s, g, tl, sl, ref["word"], r_min, True, 53)
    assert compared == 2 * 2 * C5_ENTRIES and n_traj >= N_TRAJ
    print(f"\nC5: {C5_ENTRIES} entries x 2 obstacle states, {compared} directed edges, running-sum flips {flips}; "
          f"dubins_steer_full on {len(sl)}; {n_traj} polylines row for row (longest {rows} rows)")
