"""CPU-side checks of the move-target call's boundary: include/rrtx.h declares the entry points, the library exports
them, the RRTX_TGT_* values the Python binding carries are the header's, and every host layer offers the call."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rrtx_find_new_target", "rrtx_find_new_target_dubins")


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {}
    for name in NEW:
        m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    simple, dubins = protos[NEW[0]], protos[NEW[1]]
    assert len(simple) == 14 and len(dubins) == 15
    assert [a.split()[-1].lstrip("*") for a in simple] == ["ctx", "pose", "nq", "r0", "r_stride", "r_max", "robot_radius",
                                                            "lmc", "target_idx", "edge_dist", "cost_to_goal", "radius_used",
                                                            "rounds", "status"]
    assert dubins[7] == "double r_min" and dubins[:7] + dubins[8:] == simple       # the same, plus r_min after robot_radius


def test_library_exports_them(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(hip_lib, name), name
        assert name in bound, name
    assert len(bound[NEW[0]]) == 14 and len(bound[NEW[1]]) == 15


def test_status_codes_match_the_header():
    defs = dict(re.findall(r"#define\s+(RRTX_TGT_[A-Z_]+)\s+(-?\d+)", _header()))
    assert sorted(defs) == ["RRTX_TGT_NOT_FOUND", "RRTX_TGT_OK"]
    for name, value in defs.items():
        assert getattr(_capi, name) == int(value), name
    assert _capi.RRTX_TGT_OK != _capi.RRTX_TGT_NOT_FOUND


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    for m in ("find_new_target", "find_new_target_dubins"):
        assert callable(getattr(Context, m)), m
    assert list(inspect.signature(drrt.findNewTarget).parameters)[:4] == ["S", "KD", "R", "hyberBallRad_"]
    R = drrt.RobotData([1.0, 2.0, 3.0])
    for field in ("robotPose", "nextMoveTarget", "distanceFromNextRobotPoseToNextMoveTarget", "currentMoveInvalid"):
        assert hasattr(R, field), field


def test_julia_shim_and_documents_carry_it():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    for name in NEW:
        assert f"(:{name}, LIBRRTX)" in jl, name
    assert re.search(r"function findNewTarget\(S::TS, KD::HipTree\{T\}, R::RobotData\{T\}, hyberBallRad::Float64\)", jl)
    assert 'error("unable to find a valid move target")' in jl
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "rrtx_find_new_target" in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.11\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
