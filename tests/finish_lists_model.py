"""Scenes for nn_finish_kernel's loop over "long or overflowed lists" (kernels_finish.hip): range lists of EXACT
lengths with CHOSEN node indices, and a numpy restatement of the switches the kernel and plan_radius (kernels_nn.hip)
take on them.  No GPU here; test_finish_list_scenes.py holds the scenes to their promises on the oracle alone and
test_gpu_finish_long_lists.py runs the library over them.

A cluster: the sample sits at an integer centre (centres 1000 apart on x, rows of 64 centres 1000 apart on z), the L
members of its list at distinct non-zero integer lattice offsets p with |p|^2 <= S, S the smallest bound whose ball
holds the scene's longest list, r = sqrt(S) + 0.25 for every sample of the scene.  Squared distances are exact integers,
so the stored keys sqrt(d2) are exact and ties are real.  Which lattice points a list gets is a seeded shuffle (with at
least two at the smallest |p|^2 of the list), which node index sits at which of them another: position order and index
order are unrelated, and the arrival order in the buckets is the search's own.  A sample whose list is empty is moved
off its centre by a fraction of a unit, so that its nearest node (kdFindNearest) has no equal.

The index set of every list is chosen:
  spread       a seeded random subset of the indices no other list reserves
  cons         [a, a + L)
  block        B consecutive indices from lo and the single index lo + 2048 w - 1: the bin rule of the long-list build
               (2048 equal bins of [lowest, highest]) puts w consecutive indices in a bin, so the fullest bin holds
               min(B, w).  `top` mirrors it: the single index at lo and the block at the upper end.
A list of 129 entries cannot crowd a bin with more than kFinCrowd = 128: over a range of fewer than 2048 indices every
index has a bin of its own, and over a wider one the lowest and the highest index sit in different bins.  The smallest
list that goes to the sort network for its crowd has 130 entries, 129 of them in one bin; that is the one built here.

All other nodes are uniform filler in a box around y = 5000, far from every sample."""
import numpy as np

N_NODES = 275_003
ROW = 64                    # centres per row
K_BIG, K_HUGE = 2048, 8192  # kBigSort, kHugeSort
BINS, CROWD = 2048, 128     # kFinBins, kFinCrowd
RR = 0.5                    # robot radius of the extend calls
FILLER_Y = 5000.0           # the filler's box is 1000 thick around this height
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- the kernel's and the plan's rules, restated ---------------------------------------------------------------------
def crowd(idx):
    """entries in the fullest of the 2048 index bins of a list, as nn_finish_kernel deals them (float64)"""
    idx = np.asarray(idx, dtype=np.int64)
    lo, hi = int(idx.min()), int(idx.max())
    scale = np.float64(BINS) / (np.float64(hi) - np.float64(lo) + 1.0)
    b = np.clip(((idx - lo).astype(np.float64) * scale).astype(np.int64), 0, BINS - 1)
    return int(np.bincount(b, minlength=BINS).max())


def bucket_cap(total, nq, mult):
    """plan_radius: records per sample bucket for a caller that made room for `total` entries"""
    return max(8, -(-(-(-max(total, 1) // nq) * mult) // 8) * 8)


def build(cap, nq):
    """launch_nn_finish: True = the KSORT = 8192 build"""
    return cap // nq > 512


def overflow_records(lengths, bcap):
    return int(np.maximum(0, np.asarray(lengths, dtype=np.int64) - bcap).sum())


def calls(lengths, nq, cap, n_calls, mult=2):
    """what a fresh context does call after call with the same batch and capacity: the bucket multiplier doubles (up to
    16) while the previous call left records on the overflow list, and more than 8192 of them make the next call
    scatter them in front of the finish kernel.  One dict per call: mult, bcap, overflow, prescatter, state."""
    out, prev = [], 0
    for _ in range(n_calls):
        if prev > 0 and mult < 16:
            mult *= 2
        bcap = bucket_cap(cap, nq, mult)
        ovf = overflow_records(lengths, bcap)
        pre = prev > 8192
        state = "prescattered" if pre and ovf else "gather" if ovf else "in bucket"
        out.append(dict(mult=mult, bcap=bcap, overflow=ovf, prescatter=pre, state=state))
        prev = ovf
    return out


def path(length, idx, bcap, huge):
    """the branch of nn_finish_kernel an uncut list takes: short (the half wave), placed (counting in index bins),
    network <n2>, rank (rank counting over global memory)"""
    if length <= 64 and length <= bcap:
        return "short"
    ksort = K_HUGE if huge else K_BIG
    if length > ksort:
        return "rank"
    if huge and crowd(idx) <= CROWD:
        return "placed"
    n2 = 64
    while n2 < length:
        n2 *= 2
    return f"network {n2}"


# ---- lattice ------------------------------------------------------------------------------------------------------------
def _grid():
    def make():
        k = 20
        g = np.arange(-k, k + 1)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        n2 = (p ** 2).sum(axis=1)
        keep = (n2 > 0) & (n2 <= k * k)
        p, n2 = p[keep], n2[keep]
        o = np.argsort(n2, kind="stable")
        return p[o], n2[o]
    return _once("grid", make)


def smallest_ball(longest):
    """the smallest S whose ball |p|^2 <= S holds `longest` non-zero lattice points"""
    return int(_grid()[1][longest - 1])


def lattice_ball(S):
    p, n2 = _grid()
    m = int(np.searchsorted(n2, S, side="right"))
    return p[:m], n2[:m]


def _pick(rng, ball, norms, L):
    """L lattice points of the ball in a shuffled order, at least two of them at the smallest norm of the pick"""
    o = rng.permutation(len(ball))
    take, rest = o[:L], o[L:]
    if L >= 2:
        m = norms[take].min()
        if (norms[take] == m).sum() < 2:
            spare = rest[norms[rest] == m]              # every shell of the lattice has at least six points
            out = np.flatnonzero(norms[take] != m)[-1]
            take = take.copy()
            take[out] = spare[0]
    return ball[take]


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _spread(*lengths):
    return [dict(kind="spread", L=L) for L in lengths]


def _block(B, lo, w, top=False):
    return dict(kind="block", L=B + 1, B=B, lo=lo, w=w, top=top)


def _specs(name):
    """(clusters, the hand-set workgroup as positions in that list, samples in all)"""
    if name == "huge":
        c = _spread(65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 9001)
        c += [dict(kind="cons", L=2048, a=20_000), dict(kind="cons", L=2049, a=30_000), dict(kind="cons", L=8192, a=40_000)]
        c += [_block(4096, 1_000, 128), _block(4096, 5_096, 129), _block(8191, 9_192, 129), _block(129, 500, 129, top=True)]
        c += _spread(*[(0, 1, 5, 33, 64)[i % 5] for i in range(43)])
        #        placed 8192, crowded 8192, placed 65, short (33), empty, rank counting (8193)
        return c, [11, 19, 0, 24, 21, 12], 64
    if name == "big":
        c = _spread(65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2560)
        c += _spread(*[(0, 1, 5, 33, 64, 17)[i % 6] for i in range(28)])
        #        network 2048, network 2048 (1025), network 128 (65), short (33), empty, rank counting (2560)
        return c, [14, 12, 0, 20, 17, 16], 45
    if name == "tight":
        c = _spread(*[L for _ in range(5) for L in (9, 16, 17, 33, 63, 64, 65, 200)])
        c += _spread(*[0] * (4099 - len(c)))
        return c, None, 4099
    raise KeyError(name)


def centre(c):
    return np.array([1000.0 * (c % ROW), 0.0, 1000.0 * (c // ROW)])


def scene(name):
    """dict(pts, Q, r, S, want, sets, kind, cluster_of, sph, hand): node positions, samples, the one radius, the wanted
    length and the sorted index set of every sample's list, the sample's kind, its cluster, the spheres of the flag
    tests, the first sample of the hand-set workgroup (None: no such group).  Built once, never modified."""
    def make():
        specs, hand, nq = _specs(name)
        assert len(specs) == nq
        seed = {"huge": 101, "big": 202, "tight": 303}[name]
        rng = np.random.default_rng(seed)
        S = smallest_ball(max(s["L"] for s in specs))
        ball, norms = lattice_ball(S)
        r = float(np.sqrt(np.float64(S))) + 0.25
        n = N_NODES
        taken = np.zeros(n, dtype=bool)
        sets = [None] * nq
        for c, s in enumerate(specs):                       # the chosen index sets first ...
            if s["kind"] == "cons":
                ids = np.arange(s["a"], s["a"] + s["L"])
            elif s["kind"] == "block":
                span = BINS * s["w"]
                if s["top"]:
                    ids = np.r_[s["lo"], np.arange(s["lo"] + span - s["B"], s["lo"] + span)]
                else:
                    ids = np.r_[np.arange(s["lo"], s["lo"] + s["B"]), s["lo"] + span - 1]
            else:
                continue
            assert ids.min() >= 0 and ids.max() < n and not taken[ids].any(), (name, c)
            taken[ids] = True
            sets[c] = ids
        free = rng.permutation(np.flatnonzero(~taken))       # ... then the spread ones from what is left
        at = 0
        for c, s in enumerate(specs):
            if s["kind"] == "spread":
                sets[c] = free[at:at + s["L"]]
                at += s["L"]
        filler = free[at:]
        pts = np.empty((n, 3))
        rows = (nq + ROW - 1) // ROW
        pts[filler] = np.c_[rng.uniform(0.0, 1000.0 * (ROW - 1), len(filler)), rng.uniform(FILLER_Y - 500.0, FILLER_Y + 500.0, len(filler)),
                            rng.uniform(-500.0, 1000.0 * (rows - 1) + 500.0, len(filler))]
        Qc = np.empty((nq, 3))
        sph = []
        for c, s in enumerate(specs):
            Qc[c] = centre(c)
            if s["L"] == 0:
                Qc[c] += rng.uniform(-0.4, 0.4, 3)
                continue
            pts[rng.permutation(sets[c])] = Qc[c] + _pick(rng, ball, norms, s["L"])
            # a large sphere below the cluster: its cap cuts off the lower half of the ball, the sample stays free
            delta = 0.8 + 0.3 * (c % 3)
            sph.append([Qc[c, 0], -(200.0 + delta), Qc[c, 2], 200.0])
        # sample order: a fixed shuffle of the clusters, one aligned workgroup of sixteen set by hand
        order = rng.permutation(nq)
        first = None
        if hand is not None:
            first = (nq // 16 - 1) * 16                     # the last full workgroup: its lists start late in the CSR
            others = [c for c in order if c not in hand]
            order = np.array(others[:first] + hand + others[first:])
        assert sorted(order) == list(range(nq))
        kind = [specs[c]["kind"] for c in order]
        return dict(name=name, pts=pts, Q=np.ascontiguousarray(Qc[order]), r=r, S=S,
                    want=np.array([specs[c]["L"] for c in order], dtype=np.int64),
                    sets=[np.sort(sets[c]) for c in order], kind=kind, cluster_of=order,
                    sph=np.array(sph), hand=first)
    return _once(("scene", name), make)


def normal_build_batch(name):
    """(samples, batch size): the lists of a scene that fit the LDS sort of the long-list build, and the smallest
    batch, counted in whole samples plus two, whose exact capacity still selects the normal build"""
    s = scene(name)
    keep = np.flatnonzero(s["want"] <= K_HUGE)
    return keep, int(s["want"][keep].sum()) // 513 + 3


def padded(name, keep, nq):
    """the samples `keep` of a scene followed by samples with empty balls up to nq samples in all"""
    s = scene(name)
    rng = np.random.default_rng(7 + nq)
    first = len(s["want"]) + ROW                             # centres no cluster of the scene uses
    extra = np.array([centre(first + k) + rng.uniform(-0.4, 0.4, 3) for k in range(nq - len(keep))])
    return np.ascontiguousarray(np.r_[s["Q"][keep], extra.reshape(-1, 3)])


# ---- the reference -----------------------------------------------------------------------------------------------------------
def tree(oracle, name):
    """the oracle's kd-tree of the scene, nodes inserted in index order (tight: one tree per thread -- a range search
    of the oracle costs milliseconds on a tree of this size, and tight has thousands of samples)"""
    def make():
        if name == "tight":
            return oracle.TreeSet(3, scene(name)["pts"])
        t = oracle.KDTree(3)
        t.insert_many(scene(name)["pts"])
        return t
    return _once(("tree", name), make)


def lists(oracle, name, Q):
    """range_batch of samples Q on the scene's tree"""
    return oracle.range_batch(tree(oracle, name), Q, scene(name)["r"], slice_size=64)


def lowest_nearest(ref, nq):
    """per sample (lowest node index among the entries with the smallest key, that key); (-1, inf) for an empty list"""
    ni, nd = np.full(nq, -1, dtype=np.int64), np.full(nq, np.inf)
    for j in range(nq):
        a, b = ref["offsets"][j], ref["offsets"][j + 1]
        if b > a:
            k = ref["key"][a:b]
            nd[j] = k.min()
            ni[j] = ref["idx"][a:b][k == nd[j]].min()
    return ni, nd


def reference(oracle, name):
    """the oracle's lists of the scene (range_batch: offsets, idx, key, nearest_idx, nearest_dist)"""
    return _once(("ref", name), lambda: lists(oracle, name, scene(name)["Q"]))


def reference_extend(oracle, name):
    """... with explicitEdgeCheck of both directed edges of every entry against the scene's spheres, and the nearest of
    every non-empty list by the lowest-index rule"""
    def make():
        from rrtqx_3d_amd import synth
        s, ref = scene(name), reference(oracle, name)
        p0, p1 = synth.candidate_edges(s["Q"], s["pts"], ref["offsets"], ref["idx"])
        arr, m = oracle.make_spheres(s["sph"])
        hit, _ = oracle.edges_check_spheres(arr, m, p0, p1, RR)
        k = len(ref["idx"])
        ni, nd = lowest_nearest(ref, len(s["want"]))
        return dict(ref, hit_out=hit[:k], hit_in=hit[k:], low_idx=ni, low_key=nd)
    return _once(("ext", name), make)


def table(name, n_calls=5):
    """the switches of a scene at cap = total, as text (one line per call, one per list that is not short)"""
    s = scene(name)
    nq, total = len(s["want"]), int(s["want"].sum())
    huge = build(total, nq)
    plan = calls(s["want"], nq, total, n_calls)
    lines = [f"{name}: nq {nq}, total {total}, cap // nq {total // nq}, build {K_HUGE if huge else K_BIG}, S {s['S']}"]
    for k, c in enumerate(plan):
        lines.append(f"  call {k + 1}: mult {c['mult']:2d} bcap {c['bcap']:5d} overflow {c['overflow']:6d} "
                     f"prescatter {int(c['prescatter'])} ({c['state']})")
    seen = set()
    for j in np.argsort(s["want"], kind="stable"):
        L = int(s["want"][j])
        p = [path(L, s["sets"][j], c["bcap"], huge) for c in plan]
        if L == 0 or all(x == "short" for x in p):
            continue
        row = f"  {s['kind'][j]:6s} {L:5d}: crowd {crowd(s['sets'][j]):4d}, " + " | ".join(dict.fromkeys(p))
        if row not in seen:
            seen.add(row)
            lines.append(row)
    return "\n".join(lines)
