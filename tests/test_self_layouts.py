"""The ws_self layouts of kernels_self.hip's four launchers, described as blocks (csrc/block_layout.hpp), against the
chained off_* arithmetic the launchers were written with before, copied here as Python: every field offset and every
block size must be equal, for every nq (and every k, which the closest launchers size ws_owner by).  Equal offsets are
what shows that the alignment of the fp32 shadow (float4) and of the tables did not move; equal instruction streams of
the kernels cannot.

The offsets come from a stand-alone program (tests/self_layouts_print.cpp: its own main, the block descriptions and no
HIP header) built with the host compiler; a second build with -fsanitize=address,undefined runs as a program of its own
and must print the same.

The three obstacle-table blocks (SphereTableBlock, PolygonTableBlock, PolygonGridBlock) have no earlier arithmetic to
be equal to: each table was a buffer of its own.  They are held to their rules instead: every field on a multiple of
256 bytes, the fields in declaration order and apart once their slack is counted, `bytes` the end of the last field,
the slack what the separate buffers carried, the fp32 reach groups whole."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "self_layouts_print.cpp")
NQS = (1, 2, 7, 63, 64, 65, 1000, 65537)
KS = (1, 8, 64)
# sizeof on the device side
D4, F4, I64, U64, I32, F32 = 32, 16, 8, 8, 4, 4


def reference(nq, k):
    """{(block, field): offset} by the expressions of the launchers before the blocks"""
    n, out = nq, {}
    # launch_self_join
    off_shadow = D4 * n
    off_count = off_shadow + F4 * n
    off_max = (off_count + I32 * (n + 1) + 7) & ~7
    out.update({("self_join", "tab"): 0, ("self_join", "shadow"): off_shadow, ("self_join", "count"): off_count,
                ("self_join", "absmax"): off_max, ("self_join", "bytes"): off_max + U64})
    # launch_self_join_dubins
    off_shadow = 8 * 4 * n
    off_spp = off_shadow + F4 * n
    off_count = off_spp + F32 * n
    off_max = (off_count + I32 * (n + 1) + 7) & ~7
    off_mark = off_max + U64
    b = "self_join_dubins"
    out.update({(b, "tab"): 0, (b, "shadow"): off_shadow, (b, "spp"): off_spp, (b, "count"): off_count,
                (b, "absmax"): off_max, (b, "mark"): off_mark, (b, "bytes"): off_mark + n})
    # launch_closest_self
    cap = n * k
    off_shadow = D4 * n
    off_slots = off_shadow + F4 * n
    off_rowsend = off_slots + I64 * (n + 1)
    off_max = off_rowsend + I64 * (n + 1)
    off_rows = off_max + U64
    off_near = off_rows + I32 * n
    off_rown = off_near + I32 * n
    off_nrows = off_rown + I32 * n
    b = "closest_self"
    out.update({(b, "tab"): 0, (b, "shadow"): off_shadow, (b, "slots_off"): off_slots, (b, "rows_off"): off_rowsend,
                (b, "absmax"): off_max, (b, "rows"): off_rows, (b, "tree_near"): off_near, (b, "row_owner"): off_rown,
                (b, "n_rows"): off_nrows, (b, "bytes"): off_nrows + I32, (b, "owner_bytes"): I32 * cap})
    # launch_closest_self_dubins
    off_shadow = 8 * 4 * n
    off_slots = off_shadow + F4 * n
    off_rowsend = off_slots + I64 * (n + 1)
    off_max = off_rowsend + I64 * (n + 1)
    off_spp = off_max + U64
    off_rows = off_spp + F32 * n
    off_near = off_rows + I32 * n
    off_rown = off_near + I32 * n
    off_nrows = off_rown + I32 * n
    off_mark = off_nrows + I32
    b = "closest_self_dubins"
    out.update({(b, "tab"): 0, (b, "shadow"): off_shadow, (b, "slots_off"): off_slots, (b, "rows_off"): off_rowsend,
                (b, "absmax"): off_max, (b, "spp"): off_spp, (b, "rows"): off_rows, (b, "tree_near"): off_near,
                (b, "row_owner"): off_rown, (b, "n_rows"): off_nrows, (b, "mark"): off_mark, (b, "bytes"): off_mark + n,
                (b, "owner_bytes"): I32 * cap})
    return out


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", *extra, SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    args = [str(v) for nq in NQS for k in KS for v in (nq, k)]
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        block, nq, k, field, value = line.split()
        got.setdefault((int(nq), int(k)), {})[(block, field)] = int(value)
    return got


@pytest.fixture(scope="module")
def want():
    return {(nq, k): reference(nq, k) for nq in NQS for k in KS}


@pytest.mark.parametrize("name, extra", [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined",
                                                                       "-fno-sanitize-recover=all"])])
def test_offsets_equal_the_launchers_arithmetic(tmp_path, want, name, extra):
    got = _build_and_run(tmp_path, name, extra)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        # (the plain forms print their empty spp / mark fields too: the launchers never had them, so nothing to compare)
        mine = {f: v for f, v in got[key].items() if f in want[key]}
        assert len(mine) == len(want[key]) == len(got[key]) - 4
        assert mine == want[key], (key, {f: (mine.get(f), v) for f, v in want[key].items() if mine.get(f) != v})


def test_the_layouts_are_aligned_for_their_types(want):
    """what the reference itself gives: the float4 shadow at 16, the 8-byte words at 8, the 4-byte words at 4"""
    align = dict(tab=32, shadow=16, slots_off=8, rows_off=8, absmax=8, spp=4, count=4, rows=4, tree_near=4,
                 row_owner=4, n_rows=4, mark=1)
    for key, offs in want.items():
        for (block, field), off in offs.items():
            if field in align:
                assert off % align[field] == 0, (key, block, field, off)


# ---- the obstacle tables ---------------------------------------------------------------------------------------------
NAS = (0, 1, 7, 8, 9, 64, 65535)
COUNTS = (0, 1, 300)          # vertices, path rows and ytab entries
SPHERE_FIELDS = ("rec", "reach", "reach_f", "sample", "radius", "thr_in", "orig")
POLYGON_FIELDS = ("meta", "off", "vxy", "vslope", "orig", "bbox", "pbox", "ytab", "path_off", "path")
GRID_FIELDS = ("start", "items")


def _tables(tmp_path, name, extra):
    exe = str(tmp_path / ("tables_" + name))
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", *extra, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cases = [(na, nv, rows, ny) for na in NAS for nv in COUNTS for rows in COUNTS for ny in COUNTS]
    r = subprocess.run([exe, "tables", *[str(v) for c in cases for v in c]], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    slack = dict(zip(lines[0].split()[1::2], map(int, lines[0].split()[2::2])))
    got = {}
    for line in lines[1:]:
        block, na, nv, rows, ny, field, off, count, size = line.split()
        got.setdefault((block, int(na), int(nv), int(rows), int(ny)), []).append((field, int(off), int(count), int(size)))
    assert sorted({k[1:] for k in got}) == sorted(cases) and len(got) == 3 * len(cases)
    return slack, got


@pytest.mark.parametrize("name, extra", [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined",
                                                                       "-fno-sanitize-recover=all"])])
def test_obstacle_table_blocks_keep_their_rules(tmp_path, name, extra):
    slack, got = _tables(tmp_path, name, extra)
    assert slack == dict(vxy=2, vslope=1, path=3, ytab=1, sph_aux_bytes=64, align=256)
    for (block, na, nv, rows, ny), fields in got.items():
        names = tuple(f for f, _, _, _ in fields)
        assert names == dict(spheres=SPHERE_FIELDS, polygons=POLYGON_FIELDS, grid=GRID_FIELDS)[block] + ("bytes",)
        end = 0
        for field, off, count, size in fields[:-1]:
            assert off % 256 == 0, (block, na, field, off)
            assert off >= end, (block, na, field, off, end)        # declaration order, apart from the field before
            end = off + count * size                                # (count includes the slack)
        assert fields[-1][1] == end, (block, na, fields[-1], end)  # bytes = end of the last field
        have = {f: (count, size) for f, _, count, size in fields[:-1]}
        if block == "spheres":
            want = dict(rec=(4 * na, 8), reach=(4 * na, 8), reach_f=(32 * ((na + 7) // 8), 4), sample=(8 * na, 8),
                        radius=(na + 64 // 8, 8), thr_in=(na + 64 // 8, 8), orig=(na + 64 // 4, 4))
        elif block == "polygons":
            want = dict(meta=(4 * na, 8), off=(na + 1, 4), vxy=(2 * nv + 2, 8), vslope=(nv + 1, 8), orig=(na, 4),
                        bbox=(4 * na, 8), pbox=(4 * na, 8), ytab=(ny + 1, 8), path_off=(na + 1, 4), path=(3 * rows + 3, 8))
        else:
            want = dict(start=(na + 1, 4), items=(nv, 2))
        assert have == want, (block, na, nv, rows, ny)
