"""The host layer of librrtx_hip.so -- what sizes, stages, launches and copies around the kernels -- run with no GPU
against a simulated HIP runtime (tests/hostsim/fake_hip.{hpp,cpp}), under the address and undefined-behaviour
sanitizers.  The library's 14 sources are compiled for the host alone, linked with the simulated runtime and a driver
(tests/hostsim/drive_*.cpp: its own main, calls include/rrtx.h only) into a stand-alone program; nothing is loaded into
Python and nothing touches a GPU.

The simulated runtime gives every device allocation exactly the bytes asked for, queues copies, memsets and launches per
stream and executes them when the host waits, keeps pinned and pageable host memory apart as HIP documents them, looks
every range up in the table of live blocks at the call and again at execution, and reports a copy that reads a device
byte nothing wrote.  Kernels do not run: each has a contract (tests/hostsim/contracts.cpp, with the lines of the kernel
it was read from) that says what it may read and write, and where the host reads a result back, a script that stores
one.  So this holds the host layer to its extents, lifetimes and stream order.  It does not check what a kernel
actually reads -- the contracts are a reading of the kernels -- and it does not model how the real runtime pins
pageable pages.

Each driver must end with status 0, launch the kernels named below, have copies checked, and print no finding (a
finding that has been looked at and recorded is declared by the driver, printed as KNOWN, and must come exactly once).  With
FAKEHIP_STRICT=1 pageable copies are deferred like pinned ones; what that mode reports are places that lean on the
documented behaviour of pageable copies, and it is printed, not asserted (DESIGN.md 4.9 lists them).

Measured on an 8-core host with the 8 compile jobs this test uses: cold build 12 s (14 host-only objects at -O1 -g with
both sanitizers, the runtime, the contracts, four drivers, the links); with the objects in place 0.25 s.  Drivers:
lifecycle 0.1 s, checks 4.8 s, extend 1.4 s, dubins 2.1 s; each runs twice, once in either mode."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from rrtqx_3d_amd import build as lib_build

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "hostsim")
OBJ = os.path.join(lib_build.OBJDIR, "hostsim")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
HOST_FLAGS = ["-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off"]
DRIVERS = {
    "lifecycle": ["aos_to_soa_kernel", "graph_edge_dist_kernel", "edges_spheres_kernel", "points_spheres_kernel",
                  "edges_polygons_kernel<false", "points_polygons_kernel", "points_polygons_flag_kernel"],
    "checks": ["aos_to_soa_kernel", "simple_steer_kernel", "edges_spheres_kernel", "points_spheres_kernel", "edges_polygons_kernel<false",
               "points_polygons_kernel", "points_polygons_flag_kernel"],
    "extend": ["nn_pack_kernel<3>", "nn_filter_prep_kernel<3>", "nn_scan_f32_kernel<3>", "nn_confirm_kernel<3",
               "nn_finish_kernel<3", "sample_spheres_kernel", "candidate_edges_kernel", "edges_polygons_kernel<true",
               "points_polygons_flag_kernel", "nn_nearest_f32_kernel<3>", "nn_nearest_out_kernel"],
    "dubins": ["nn_pack_kernel<4>", "nn_filter_prep_kernel<4>", "nn_scan_f32_kernel<4>", "nn_confirm_kernel<4",
               "nn_finish_kernel<4", "dubins_steer_rec_kernel", "dubins_check_rec_kernel<false", "dubins_check_rec_kernel<true",
               "points_polygons_flag_kernel", "nn_nearest_f32_kernel<4>", "nn_nearest_out_kernel"],
}
# copies each driver has checked at the least (what it does today; a driver that stops reaching the code falls below)
COPIES = {"lifecycle": 500, "checks": 1850, "extend": 700, "dubins": 1000}
JOBS = 8


def _tools():
    hipcc = lib_build.HIPCC if os.path.exists(lib_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc: the host-only objects cannot be built")
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), os.environ.get("ROCM_PATH", "/opt/rocm")]
    clang = next((c for r in roots for c in (os.path.join(r, "lib", "llvm", "bin", "clang++"), os.path.join(r, "llvm", "bin", "clang++"))
                  if os.path.exists(c)), None)
    if not clang:
        pytest.skip("no clang++ beside hipcc: the drivers must link with the compiler that built the objects")
    nm = shutil.which("nm") or os.path.join(os.path.dirname(clang), "llvm-nm")
    include = next((os.path.join(r, "include") for r in roots if os.path.exists(os.path.join(r, "include", "hip"))), None)
    return hipcc, clang, nm, include


def _stale(obj, deps):
    return any(lib_build._newer(d, obj) for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout[-3000:] + r.stderr[-3000:]


def build_drivers():
    """{driver name: program}; objects newer than their sources and headers are kept, as rrtqx_3d_amd/build.py does"""
    hipcc, clang, nm, include = _tools()
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.normpath(os.path.join(lib_build.CSRC, h)) for h in lib_build.HEADERS]
    sim_headers = [os.path.join(SIM, h) for h in ("fake_hip.hpp", "contracts.hpp", "drive_common.hpp")]
    hip_host = [hipcc, "--cuda-host-only", "--offload-arch=gfx950", *HOST_FLAGS, "-Wno-unused-function",
                *[f for s in SAN for f in ("-Xarch_host", s)]]
    plain = [clang, *HOST_FLAGS, *SAN, "-D__HIP_PLATFORM_AMD__", "-I", include]
    jobs = []
    for src in lib_build.SOURCES:
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        path = os.path.join(lib_build.CSRC, src)
        jobs.append((obj, [path] + headers, hip_host + ["-c", path, "-o", obj]))
    path = os.path.join(SIM, "contracts.cpp")
    jobs.append((os.path.join(OBJ, "contracts.o"), [path] + headers + sim_headers,
                 hip_host + ["-x", "hip", "-c", path, "-o", os.path.join(OBJ, "contracts.o")]))
    for name in ["fake_hip"] + ["drive_" + d for d in DRIVERS]:
        path = os.path.join(SIM, name + ".cpp")
        jobs.append((os.path.join(OBJ, name + ".o"), [path] + sim_headers, plain + ["-c", path, "-o", os.path.join(OBJ, name + ".o")]))
    with ThreadPoolExecutor(max_workers=JOBS) as ex:
        list(ex.map(lambda j: _run(j[2]) if _stale(j[0], j[1]) else None, jobs))
    lib_objs = [j[0] for j in jobs if not os.path.basename(j[0]).startswith(("fake_hip", "drive_"))]
    # every host-only object refers to the device code it would carry as one data symbol, __hip_fatbin_<hash>: define
    # exactly the names the objects ask for, so that any other missing symbol still fails the link
    r = subprocess.run([nm, "-u", *lib_objs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = sorted({w for line in r.stdout.splitlines() for w in line.split() if w.startswith("__hip_fatbin_")})
    assert len(names) >= len(lib_build.SOURCES), names
    fat_src, fat_obj = os.path.join(OBJ, "fatbin_symbols.cpp"), os.path.join(OBJ, "fatbin_symbols.o")
    text = "".join('extern "C" { extern const char %s[8]; const char %s[8] = {0}; }\n' % (n, n) for n in names)
    if not os.path.exists(fat_src) or open(fat_src).read() != text:
        with open(fat_src, "w") as f:
            f.write(text)
    if _stale(fat_obj, [fat_src]):
        _run([clang, "-c", fat_src, "-o", fat_obj])
    programs = {}
    for d in DRIVERS:
        exe = os.path.join(OBJ, "drive_" + d)
        objs = lib_objs + [fat_obj, os.path.join(OBJ, "fake_hip.o"), os.path.join(OBJ, "drive_" + d + ".o")]
        if _stale(exe, objs):
            _run([clang, *SAN, "-o", exe, *objs, "-ldl", "-lpthread"])
        programs[d] = exe
    return programs


@pytest.fixture(scope="module")
def programs():
    return build_drivers()


def _drive(exe, strict):
    env = dict(os.environ, FAKEHIP_STRICT="1" if strict else "0")
    r =subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    lines = r.stdout.splitlines()
    return r, lines, [ln for ln in lines if ln.startswith("FINDING ")]


@pytest.mark.parametrize("driver", sorted(DRIVERS))
def test_driver_runs_clean(programs, driver):
    r, lines, found = _drive(programs[driver], strict=False)
    tail = "\n".join(lines[-40:]) + r.stderr[-3000:]
    assert not found, "\n".join(found[:20])
    assert r.returncode == 0, tail
    launches = {ln.split("   <- ")[0].split(" ", 2)[2]: int(ln.split()[1]) for ln in lines if ln.startswith("LAUNCH ")}
    for part in DRIVERS[driver]:
        assert any(part in name and n > 0 for name, n in launches.items()), (part, sorted(launches))
    assert not [ln for ln in lines if ln.startswith("LAUNCH ") and ln.endswith("NO CONTRACT")], tail
    counts = dict(ln.split() for ln in lines if ln.split()[0] in ("COPIES", "LIVE_BLOCKS", "KNOWN_FINDINGS", "FINDINGS"))
    assert int(counts["COPIES"]) >= COPIES[driver] and counts["FINDINGS"] == "0", counts
    assert counts["LIVE_BLOCKS"] == "0", counts          # every context was destroyed: nothing of it is left
    # findings that were looked at and recorded: the extend driver's six first calls that leave out an
    # optional per-sample output, whose column of the block then travels unwritten and unread
    assert int(counts["KNOWN_FINDINGS"]) == (6 if driver == "extend" else 0), counts


@pytest.mark.parametrize("driver", sorted(DRIVERS))
def test_driver_strict_mode_reports(programs, driver):
    """deferred pageable copies: the sanitizers stay silent and the driver ends by its own count (0, or 3 = findings);
    the findings are places that lean on documented behaviour, printed here and listed in DESIGN.md 4.9"""
    r, lines, found = _drive(programs[driver], strict=True)
    print("\n".join(sorted({ln.split("[")[0] for ln in found})))
    assert r.returncode in (0, 3), "\n".join(lines[-40:]) + r.stderr[-3000:]
    assert (r.returncode == 3) == bool(found)
