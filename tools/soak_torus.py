"""Soak of the wrapped searches on lattice tori (tests/torus_model.py): up to three wrapped dimensions, so up to eight
copies per query, periods that are powers of two, so queries sit exactly on period / 2, ghosts exactly on the skip
threshold and nodes exactly at r.  The range search under its switches, the nearest search three ways, the fused Dubins
preamble, findNewTarget and the polygon sweeps with their ghost queries, through the C-ABI against the oracle, bit for
bit.  The check_* functions are the comparisons of tests/test_gpu_torus.py; scene(seed) draws the space they run on."""
import math
import os
import sys
import time

import numpy as np

import torch                            # before the library is loaded: _capi.load() then brings PyTorch's runtime up first

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, ".."))
sys.path.insert(0, os.path.join(_HERE, "..", "tests"))
import torus_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402
from rrtqx_3d_amd import _capi  # noqa: E402
from rrtqx_3d_amd.context import Context  # noqa: E402

RR, RMIN = 0.25, 0.5                    # robot radius and minimum turning radius of the Dubins scenes
VMIN, VMAX = 1.0, 8.0                   # validMove's velocity window in the space with time
SWITCHES = [(cull, filt, tune) for cull in (0, 2) for filt in (0, 1) for tune in (0, 8)]
BATCHES = (1, 2, 33)                    # prefixes of the queries: nq x 2^w copies end inside and across tiles


class Ref:
    """The oracle's answers for one scene, each computed once: range lists per radius (ascending node index, as the
    device returns them) and kdFindNearest"""

    def __init__(self, sc):
        self.sc = sc
        self.trees = O.TreeSet(sc["dim"], sc["nodes"], wraps=list(sc["wraps"]), wrap_points=list(sc["periods"]))
        self._lists = {}
        self._nearest = None

    def lists(self, r):
        key = "mix" if np.ndim(r) else float(r)
        if key not in self._lists:
            self._lists[key] = O.range_batch(self.trees, self.sc["Q"], r, nearest=False)
        return self._lists[key]

    def nearest(self):
        if self._nearest is None:
            t = self.trees.trees[0]
            self._nearest = np.array([t.nearest(q)[1] for q in self.sc["Q"]])
        return self._nearest


def radii_of(sc):
    return [(str(r), r) for r in sc["radii"]] + [("mix", sc["r_mix"])]


def make_ctx(sc, options=(), upto=None):
    ctx = Context(sc["dim"])
    try:
        for opt, val in options:
            ctx.set_option(opt, val)
        for d, per in zip(sc["wraps"], sc["periods"]):
            ctx.set_wrap(d, per)
        ctx.nodes_append(sc["nodes"][:upto])
    except Exception:
        ctx.close()
        raise
    return ctx


def prefix(ref, b):
    n = int(ref["offsets"][b])
    return dict(offsets=ref["offsets"][:b + 1], idx=ref["idx"][:n], key=ref["key"][:n])


def assert_lists(got, want, label):
    off, idx, dist = got
    O.assert_same_results(dict(offsets=off, idx=idx, key=dist), want, ("offsets", "idx", "key"), label=label + ": ")


def check_radius(ctx, sc, ref, label, batches=BATCHES, radii=None):
    """nn_radius on every radius of the scene (scalars and the per-query array), all queries; the prefixes of `batches`
    at the two radii whose lists differ most.  Returns the neighbours compared."""
    total = 0
    nq = len(sc["Q"])
    for name, r in (radii_of(sc) if radii is None else radii):
        want = ref.lists(r)
        assert_lists(ctx.nn_radius(sc["Q"], r), want, f"{label} r={name}")
        total += len(want["idx"])
        if name in ("3.25", "mix"):
            for b in batches:
                if b < nq:
                    rb = r[:b] if np.ndim(r) else r
                    assert_lists(ctx.nn_radius(sc["Q"][:b], rb), prefix(want, b), f"{label} r={name} nq={b}")
    return total


def check_nearest_result(sc, ref, idx, dist, label):
    """the distance is kdFindNearest's bit for bit; index ties are legitimate on a lattice, so the index is held to
    this: some copy of the query has exactly that distance to that node"""
    want = ref.nearest()
    assert np.array_equal(dist.view(np.uint64), want.view(np.uint64)), f"{label}: nearest distances differ"
    assert ((idx >= 0) & (idx < len(sc["nodes"]))).all(), f"{label}: nearest index out of range"
    d = M.copy_dists(sc["nodes"][idx], sc["Q"], sc["wraps"], sc["periods"])
    assert (d == want[None]).any(axis=0).all(), f"{label}: a nearest index is not at the nearest distance"


def check_nearest(sc, ref, label, dev=True):
    """nn_nearest: default, the exact scan (NN_FILTER 0), and a record buffer of 64 so that the fix-up kernel answers;
    nn_nearest_dev with that buffer"""
    for name, options in (("default", ()), ("exact", ((_capi.RRTX_OPT_NN_FILTER, 0),)),
                          ("fixup", ((_capi.RRTX_OPT_NEAREST_REC_CAP, 64),))):
        with make_ctx(sc, options) as ctx:
            idx, dist = ctx.nn_nearest(sc["Q"])
            check_nearest_result(sc, ref, idx, dist, f"{label} nearest {name}")
            if name == "fixup" and dev:
                d = torch.device("cuda", 0)
                nq = len(sc["Q"])
                d_q = torch.from_numpy(np.array(sc["Q"])).to(d)
                d_i = torch.full((nq,), -9, dtype=torch.int32, device=d)
                d_d = torch.empty(nq, dtype=torch.float64, device=d)
                torch.cuda.synchronize()
                ctx.nn_nearest_dev(d_q.data_ptr(), nq, d_i.data_ptr(), d_d.data_ptr())
                ctx.sync()
                check_nearest_result(sc, ref, d_i.cpu().numpy(), d_d.cpu().numpy(), f"{label} nearest_dev fixup")


def lattice_polygons(rng, m, span):
    """boxes and right triangles with lattice corners inside [0, span]^2"""
    polys = []
    for j in range(m):
        c = rng.integers(0, int(4 * span) - 4, 2) / 4.0
        w, h = rng.integers(1, 5, 2) / 4.0
        polys.append(c + np.array([[0, 0], [w, 0], [w, h], [0, h]] if j % 2 == 0 else [[0, 0], [w, 0], [0, h]], dtype=np.float64))
    return polys


def check_dubins(sc, ref, label, radii=(2.5, 3.75), has_time=False, target=True, seed=0):
    """extend_candidates_dubins in a dim 4 scene: lists and keys against the wrapped oracle tree, costs, words and flag
    bytes against dubins_candidates_batch on those lists, nearest against the tree; find_new_target_dubins on the same
    context against find_target_batch.  Returns the entries compared."""
    from test_find_target_reference import KEYS, Scene, find_target_batch
    rng = np.random.default_rng(M.SEED + 700 + seed)
    polys = lattice_polygons(rng, 6, 5.0)
    ps = O.PolygonSet(polys)
    mode = dict(has_time=has_time, piecewise=has_time, v_min=VMIN if has_time else 0.0, v_max=VMAX if has_time else 0.0)
    nodes, Q = sc["nodes"], sc["Q"]
    total = 0
    with make_ctx(sc) as ctx:
        ctx.polygons_set(polys)
        if has_time:
            ctx.set_space_has_time(True)
            ctx.set_dubins_velocity(VMIN, VMAX)
        for r in radii:
            want = dict(ref.lists(r))
            got = ctx.extend_candidates_dubins(Q, r, RR, RMIN)
            O.assert_same_results(got, want, ("offsets", "idx", "key"), label=f"{label} dubins r={r}: ")
            c = O.dubins_candidates_batch(Q, want["offsets"], want["idx"], nodes, RMIN, ps, RR, **mode)
            owner = np.repeat(np.arange(len(Q)), np.diff(want["offsets"]))
            eo = O.dubins_edges_batch(Q[owner], nodes[want["idx"]], RMIN, has_time=has_time, piecewise=has_time)
            ei = O.dubins_edges_batch(nodes[want["idx"]], Q[owner], RMIN, has_time=has_time, piecewise=has_time)
            want.update(cost_out=c["cost_out"], cost_in=c["cost_in"], hit_out=c["hit_out"], hit_in=c["hit_in"],
                        word_out=eo["word"], word_in=ei["word"])
            for k in ("cost_out", "cost_in", "hit_out", "hit_in", "word_out", "word_in"):
                assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), f"{label} dubins r={r}: {k} differ"
            check_nearest_result(sc, ref, got["nearest_idx"], got["nearest_dist"], f"{label} dubins r={r}")
            total += len(want["idx"])
        if target:
            scene = Scene("dubins_time" if has_time else "dubins", nodes, ps, RR, r_min=RMIN, v_min=mode["v_min"],
                          v_max=mode["v_max"], wraps=list(sc["wraps"]), wrap_points=list(sc["periods"]))
            lmc = rng.integers(0, 40, len(nodes)) / 4.0
            lmc[rng.random(len(nodes)) < 0.5] = math.inf
            lmc[0] = 0.0
            r0 = sc["r_mix"] / 2.0
            want = find_target_batch(O, scene, ref.trees, Q, r0, 5.0, lmc)
            got = ctx.find_new_target_dubins(Q, r0, 5.0, RR, RMIN, lmc=lmc)
            for k in KEYS:
                assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), f"{label} find_new_target: {k} differ"
    return total


def check_sweeps(sc, label):
    """obstacle_sweep_polygon (mode 0) and obstacle_sweep_polygon_batch on a planar torus against
    add_new_obstacle_edges over a wrapped tree.  Returns the edges compared."""
    nodes, polys, es, ee = sc["nodes"], sc["polys"], sc["es"], sc["ee"]
    ps = O.PolygonSet(polys)
    tree = O.KDTree(sc["dim"], list(sc["wraps"]), list(sc["periods"]))
    tree.insert_many(nodes)
    m = len(polys)
    want = [O.add_new_obstacle_edges(tree, nodes, es, ee, ps, j, M.SWEEP_RR, M.SWEEP_DELTA, dubins=False) for j in range(m)]
    with make_ctx(sc) as ctx:
        ctx.polygons_set(polys)
        assert ctx.graph_edges_append(es, ee) == 0
        for j in range(m):
            got = ctx.obstacle_sweep_polygon(j, M.SWEEP_RR, M.SWEEP_DELTA, cap=8)
            assert np.array_equal(got, want[j]), f"{label} sweep of obstacle {j} differs"
        order = list(range(m - 1, -1, -1))
        off, ids = ctx.obstacle_sweep_polygon_batch(order, M.SWEEP_RR, M.SWEEP_DELTA, cap=8)
        assert off[0] == 0 and off[-1] == len(ids)
        for row, j in enumerate(order):
            assert np.array_equal(ids[off[row]:off[row + 1]], want[j]), f"{label} batch row of obstacle {j} differs"
    return want


def scene(seed):
    """draws the space (dim 3 or 4, two or three wrapped dimensions, periods from {2, 4, 8}, the wrap order), the node
    count and the queries; runs the range search under every switch, the nearest search, and the sweeps on a planar
    torus; every fourth scene is a Dubins space [x y t theta] with theta and t wrapped and runs the fused preamble"""
    rng = np.random.default_rng(M.SEED + 3000 + seed)
    out = dict(nbrs=0, dubins=0, sweep_edges=0, copies8=0)
    if seed % 4 == 3:
        sp = dict(dim=4, wraps=(3, 2) if seed % 8 == 3 else (2, 3), span=5.0, n=int(rng.choice([300, 900])), nq=32)
        sp["periods"] = tuple(M.TWO_PI if d == 3 else 4.0 for d in sp["wraps"])
    else:
        dim = int(rng.choice([3, 4]))
        w = int(rng.choice([2, 3]))
        wraps = tuple(int(d) for d in rng.permutation(dim)[:w])
        sp = dict(dim=dim, wraps=wraps, periods=tuple(float(p) for p in rng.choice([2.0, 4.0, 8.0], w)), span=4.0,
                  n=int(rng.choice([300, 2000, 5000])), nq=int(rng.choice([33, 128, 256])))
    sc = M.build(sp, rng, f"soak{seed}")
    ref = Ref(sc)
    label = f"scene {seed} {sp['dim']}-D wraps {sp['wraps']} periods {sp['periods']}"
    out["copies8"] = int(M.searched(sc["Q"], 3.75, sc["wraps"], sc["periods"]).all(axis=0).sum()) if len(sp["wraps"]) == 3 else 0
    for cull, filt, tune in SWITCHES:
        opts = ((_capi.RRTX_OPT_NN_CULL, cull), (_capi.RRTX_OPT_NN_FILTER, filt), (_capi.RRTX_OPT_TUNE, tune))
        with make_ctx(sc, opts) as ctx:
            out["nbrs"] += check_radius(ctx, sc, ref, f"{label} cull={cull} filter={filt} tune={tune}")
    # nodes inside [0, period] (what the model draws): kdFindNearest is the minimum over all copies
    check_nearest(sc, ref, label)
    if seed % 4 == 3:
        out["dubins"] += check_dubins(sc, ref, label, radii=(float(rng.choice([2.5, 3.25])),), has_time=seed % 8 == 7,
                                      seed=seed)
    want = check_sweeps(M.planar_scene(seed + 1), label)
    out["sweep_edges"] += sum(len(w) for w in want)
    return out


if __name__ == "__main__":
    n_scen = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    t0 = time.time()
    tot = {}
    failed = []
    for s in range(n_scen):
        try:
            o = scene(s)
        except AssertionError as err:               # a comparison that differs: say which, go on, fail at the end
            print(f"DIFFERS: {err}", flush=True)
            failed.append(s)
            continue
        for k in o:
            tot[k] = tot.get(k, 0) + o[k]
        if (s + 1) % 10 == 0:
            print(f"{s + 1} scenes ok, {tot}, {time.time() - t0:.0f} s", flush=True)
    print("SOAK OK" if not failed else f"SOAK FAILED in scenes {failed}", n_scen, tot, f"{time.time() - t0:.0f} s")
    sys.exit(1 if failed else 0)
