"""The scenes of finish_lists_model.py keep their promises -- judged on the CPU oracle and a numpy restatement alone,
so that test_gpu_finish_long_lists.py can hold the library to them: exact lengths and index sets, exact keys with ties
at the minimum, every switch of nn_finish_kernel and plan_radius taken on the side the scene names, and spheres that
flag about half of every long list."""
import numpy as np
import pytest

import finish_lists_model as M

SCENES = ("huge", "big", "tight")


def spec(name, kind, L):
    """the one sample of the scene with this kind and list length"""
    s = M.scene(name)
    hits = [j for j in range(len(s["want"])) if s["kind"][j] == kind and s["want"][j] == L]
    assert len(hits) == 1, (name, kind, L, hits)
    return hits[0]


@pytest.mark.parametrize("name", SCENES)
def test_lists_are_the_chosen_ones(oracle, name):
    s, ref = M.scene(name), M.reference(oracle, name)
    t = M.tree(oracle, name)
    assert len(s["pts"]) == M.N_NODES and (t.trees[0] if name == "tight" else t).depth() < 100
    assert np.array_equal(np.diff(ref["offsets"]), s["want"])
    for j, ids in enumerate(s["sets"]):
        assert np.array_equal(ref["idx"][ref["offsets"][j]:ref["offsets"][j + 1]], ids), (name, j)
    assert len(np.unique(s["Q"], axis=0)) == len(s["Q"])
    # position order and index order are unrelated: no long list is monotone in any coordinate
    for j in np.flatnonzero(s["want"] > 64):
        p = s["pts"][s["sets"][j]]
        assert all((np.diff(p[:, k]) < 0).any() and (np.diff(p[:, k]) > 0).any() for k in range(3)), (name, j)


@pytest.mark.parametrize("name", SCENES)
def test_lists_equal_an_all_pairs_restatement(oracle, name):
    """(dx^2 + dy^2) + dz^2 < r^2 on exact integers, keys sqrt: huge and big over every (sample, node) pair; tight over
    every pair of its samples with the cluster nodes and of a hundred samples with all nodes -- the filler is further
    than r from EVERY sample in y alone, which is asserted"""
    s, ref = M.scene(name), M.reference(oracle, name)
    pts, Q, r = s["pts"], s["Q"], s["r"]
    nq = len(Q)
    near = np.flatnonzero(pts[:, 1] < 100.0)                       # cluster nodes
    far = np.flatnonzero(pts[:, 1] >= 100.0)
    assert len(near) == s["want"].sum()
    assert (pts[far, 1].min() - Q[:, 1].max()) ** 2 >= r * r and np.abs(Q[:, 1]).max() < 1.0
    assert (pts[near] == np.rint(pts[near])).all() and s["S"] < r * r < s["S"] + 7
    every = np.arange(len(pts))
    if name == "tight":
        rng = np.random.default_rng(1)
        full = set(np.flatnonzero(s["want"] > 0)) | set(rng.choice(nq, 60, replace=False))
    else:
        full = set(range(nq))
    for j in range(nq):
        cand = every if j in full else near
        d = pts[cand] - Q[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inb = np.flatnonzero(d2 < r * r)
        a, b = ref["offsets"][j], ref["offsets"][j + 1]
        assert np.array_equal(cand[inb], ref["idx"][a:b]), (name, j)
        assert np.array_equal(np.sqrt(d2[inb]).view(np.int64), ref["key"][a:b].view(np.int64)), (name, j)
        if len(inb):
            assert (d2[inb] == np.rint(d2[inb])).all() and d2[inb].max() <= s["S"]


@pytest.mark.parametrize("name", SCENES)
def test_ties_at_the_minimum(oracle, name):
    """every list of more than 64 entries has at least two entries at its smallest key, at unrelated node indices"""
    s, ref = M.scene(name), M.reference(oracle, name)
    low_i, low_k = M.lowest_nearest(ref, len(s["want"]))
    gaps = []
    for j in np.flatnonzero(s["want"] > 64):
        a, b = ref["offsets"][j], ref["offsets"][j + 1]
        k = ref["key"][a:b]
        tied = ref["idx"][a:b][k == k.min()]
        assert len(tied) >= 2 and low_k[j] == k.min() == np.sqrt(np.rint(k.min() ** 2)) and low_i[j] == tied.min()
        gaps.append(int(tied.max() - tied.min()))
    assert min(gaps) >= 1 and (name == "tight" or np.median(gaps) > 1000)
    for j in np.flatnonzero(s["want"] == 0):
        assert low_i[j] == -1 and 0 <= ref["nearest_idx"][j] < M.N_NODES


def test_huge_takes_every_switch(oracle):
    s = M.scene("huge")
    want, nq, total = s["want"], len(s["want"]), int(s["want"].sum())
    assert nq == 64 and M.build(total, nq) and total // nq > 512
    assert sorted(want[want > 64]) == sorted([65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193,
                                              9001, 2048, 2049, 8192, 4097, 4097, 8192, 130])
    assert sorted(set(want[want <= 64])) == [0, 1, 5, 33, 64]
    assert s["S"] == M.smallest_ball(9001) and len(M.lattice_ball(156)[0]) == 8216
    # the crowd rule, on both sides of kFinCrowd
    w128, w129 = [j for j in range(nq) if s["kind"][j] == "block" and want[j] == 4097]
    if M.crowd(s["sets"][w128]) != 128:
        w128, w129 = w129, w128
    assert M.crowd(s["sets"][w128]) == M.CROWD == 128 and M.crowd(s["sets"][w129]) == 129

    def span(j):
        return int(s["sets"][j][-1] - s["sets"][j][0] + 1)
    assert span(w128) == 2048 * 128 and span(w129) == 2048 * 129
    c8192, c130 = spec("huge", "block", 8192), spec("huge", "block", 130)
    assert M.crowd(s["sets"][c8192]) == 129 and M.crowd(s["sets"][c130]) == 129
    plan = M.calls(want, nq, total, 5)
    bcap = plan[-1]["bcap"]
    assert M.path(4097, s["sets"][w128], bcap, True) == "placed"
    assert M.path(4097, s["sets"][w129], bcap, True) == "network 8192"
    assert M.path(8192, s["sets"][c8192], bcap, True) == "network 8192"
    assert M.path(130, s["sets"][c130], bcap, True) == "network 256"
    for j in range(nq):
        if s["kind"][j] != "block" and 64 < want[j] <= 8192:
            assert M.crowd(s["sets"][j]) <= 32 and M.path(want[j], s["sets"][j], bcap, True) == "placed", j
        if s["kind"][j] == "cons":
            assert M.crowd(s["sets"][j]) <= 4 and (np.diff(s["sets"][j]) == 1).all()
    assert M.path(8193, s["sets"][spec("huge", "spread", 8193)], bcap, True) == "rank"
    assert M.path(9001, s["sets"][spec("huge", "spread", 9001)], bcap, True) == "rank"
    # the calls of one context: gathered in the kernel, pre-scattered and still overflowing, all in the buckets
    assert [c["state"] for c in plan] == ["gather", "prescattered", "in bucket", "in bucket", "in bucket"]
    assert [c["mult"] for c in plan] == [2, 4, 8, 8, 8]
    assert [c["prescatter"] for c in plan] == [False, True, True, False, False]
    assert plan[0]["overflow"] > 8192 and plan[1]["overflow"] > 8192 and plan[2]["overflow"] == 0
    assert plan[0]["bcap"] == M.bucket_cap(total, nq, 2) == (-(-total // nq) * 2 + 7) // 8 * 8
    assert M.calls(want, nq, total, 1, mult=16)[0]["overflow"] == 0
    # the workgroup set by hand
    h = s["hand"]
    assert h % 16 == 0 and h + 16 <= nq and list(want[h:h + 6]) == [8192, 8192, 65, 33, 0, 8193]
    assert [M.path(want[h + k], s["sets"][h + k], bcap, True) if want[h + k] else "empty" for k in range(6)] == \
        ["placed", "network 8192", "placed", "short", "empty", "rank"]


def test_big_takes_every_switch(oracle):
    s = M.scene("big")
    want, nq, total = s["want"], len(s["want"]), int(s["want"].sum())
    assert not M.build(total, nq) and nq % 16
    assert sorted(want[want > 64]) == [65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
                                       2049, 2560]
    plan = M.calls(want, nq, total, 5)
    assert plan[0]["state"] == "gather" and plan[0]["overflow"] <= 8192 and not any(c["prescatter"] for c in plan)
    assert plan[-1]["state"] == "in bucket"
    bcap = plan[-1]["bcap"]
    got = {int(L): M.path(L, s["sets"][j], bcap, False) for j, L in enumerate(want) if L > 64}
    assert got == {65: "network 128", 127: "network 128", 128: "network 128", 129: "network 256", 255: "network 256",
                   256: "network 256", 257: "network 512", 511: "network 512", 512: "network 512", 513: "network 1024",
                   1023: "network 1024", 1024: "network 1024", 1025: "network 2048", 2047: "network 2048",
                   2048: "network 2048", 2049: "rank", 2560: "rank"}
    h = s["hand"]
    assert h % 16 == 0 and list(want[h:h + 6]) == [2048, 1025, 65, 33, 0, 2560]
    # the same lists in the other build: a capacity padded to more than 512 entries a sample
    cap = 513 * nq
    assert cap >= total and M.build(cap, nq)
    assert all(M.path(L, s["sets"][j], M.bucket_cap(cap, nq, 2), True) == "placed" for j, L in enumerate(want) if L > 64)


def test_tight_overflows_every_list(oracle):
    s = M.scene("tight")
    want, nq, total = s["want"], len(s["want"]), int(s["want"].sum())
    assert nq == 4099 and (want > 0).sum() == 40 and not M.build(total, nq)
    assert sorted(set(want[want > 0])) == [9, 16, 17, 33, 63, 64, 65, 200]
    plan = M.calls(want, nq, total, 5)
    assert [c["bcap"] for c in plan] == [8, 8, 8, 16, 16] and [c["mult"] for c in plan] == [2, 4, 8, 16, 16]
    assert all(c["state"] == "gather" and 0 < c["overflow"] <= 8192 for c in plan)
    assert plan[0]["overflow"] == total - 8 * 40
    paths = {int(L): M.path(L, s["sets"][j], 8, False) for j, L in enumerate(want) if L > 0}
    assert paths == {9: "network 64", 16: "network 64", 17: "network 64", 33: "network 64", 63: "network 64",
                     64: "network 64", 65: "network 128", 200: "network 256"}
    assert len(set(np.flatnonzero(want > 0) // 16)) >= 30          # the lists sit in many different workgroups


def test_huge_lists_fit_the_normal_build(oracle):
    """the lists of huge that are no longer than 8192, padded with empty balls until cap // nq <= 512"""
    s = M.scene("huge")
    keep, nq = M.normal_build_batch("huge")
    total = int(s["want"][keep].sum())
    assert len(keep) == 62 and not M.build(total, nq) and M.build(total, nq - 3)
    Q = M.padded("huge", keep, nq)
    ref = M.lists(oracle, "huge", Q)
    assert np.array_equal(np.diff(ref["offsets"]), np.r_[s["want"][keep], np.zeros(nq - len(keep), dtype=np.int64)])
    assert np.array_equal(ref["idx"], np.concatenate([s["sets"][j] for j in keep]))


@pytest.mark.parametrize("name", SCENES)
def test_spheres_flag_about_half_of_every_long_list(oracle, name):
    s, ext = M.scene(name), M.reference_extend(oracle, name)
    arr, m = oracle.make_spheres(s["sph"])
    unsafe, _ = oracle.points_check_spheres(arr, m, s["Q"], M.RR)
    assert not unsafe.any()
    for j in np.flatnonzero(s["want"] > 8):
        a, b = ext["offsets"][j], ext["offsets"][j + 1]
        for f in ("hit_out", "hit_in"):
            assert 0.2 <= ext[f][a:b].mean() <= 0.8, (name, j, f)
