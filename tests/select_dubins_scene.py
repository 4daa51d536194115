"""The scene of the rrtx_extend_select_dubins tests: a Context(4) with theta wrapped, 2 000 nodes of synth.nodes and
the polygons of synth.polygons, or (has_time) the kind-6 polygons and paths of rand_StaticTime_7 with the velocities of
tests/test_gpu_extend_select.py::test_dubins_lists.  Radii are chosen from numpy distances in the wrapped space so that
the mean row length of a batch is a number given in advance (the lanes walk_group gives a sample follow from it)."""
import json
import math
import os

import numpy as np

from rrtqx_3d_amd import synth
from rrtqx_3d_amd.context import Context

HERE = os.path.dirname(os.path.abspath(__file__))
N, POOL, RR = 2000, 256, 0.5
TWO_PI = 2.0 * math.pi
# walk_group (csrc/list_walk.hpp): mean = entries // samples; 8 lanes up to a mean of 8, 16 up to 16, 32 up to 32, else 64.
# The mean row length aimed at for each group width, in the middle of its band.
MEAN_FOR_GROUP = {8: 6, 16: 12, 32: 24, 64: 48}


def group_of(offsets):
    nq = len(offsets) - 1
    mean = int(offsets[-1]) // max(nq, 1)
    g = 8
    while g < 64 and g < mean:
        g *= 2
    return g


def r_min_of(has_time):
    return 2.0 if has_time else 1.0


def points(has_time):
    """(nodes, the pool of samples)"""
    rng = np.random.default_rng(23)
    pts, Q = synth.nodes(N, 4), synth.queries(POOL, 4)
    if has_time:
        pts[:, 2] = rng.uniform(10.0, 35.0, N)
        Q[:, 2] = rng.uniform(10.0, 35.0, POOL)
    return pts, Q


def lmc_values():
    """rrtLMC per node: about a tenth +Inf, the root at 0"""
    rng = np.random.default_rng(29)
    lmc = rng.uniform(0.0, 80.0, N)
    lmc[rng.random(N) < 0.1] = math.inf
    lmc[0] = 0.0
    return lmc


def context(has_time):
    pts, _ = points(has_time)
    ctx = Context(4)
    ctx.set_wrap(3, TWO_PI)
    ctx.nodes_append(pts)
    if has_time:
        env = json.load(open(os.path.join(HERE, "golden", "env_inputs.json")))
        polys = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_polygons"]][::-1]
        paths = [np.array(p, dtype=np.float64) for p in env["rand_StaticTime_7_paths"]][::-1]
        ctx.polygons_set(polys, kinds=[6] * len(polys), paths=paths)
        ctx.set_space_has_time(True)
        ctx.set_dubins_velocity(5.0, 30.0)
    else:
        ctx.polygons_set(synth.polygons(24))
    return ctx


def radius_for(Q, pts, total):
    """A radius with exactly `total` (sample, node) pairs inside: half way between the total-th and the next pair
    distance, theta taken the short way round."""
    d = Q[:, None, :] - pts[None, :, :]
    th = np.abs(d[..., 3])
    d[..., 3] = np.minimum(th, TWO_PI - th)
    dist = np.sort(np.sqrt((d * d).sum(axis=2)).ravel())
    return 0.5 * (dist[total - 1] + dist[total])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
