"""CPU-side checks of the batched polygon release's boundary: include/rrtx.h declares rrtx_obstacle_release_polygon_batch
and rrtx_polygons_set_active, the library exports them, the Python binding carries them with the header's eleven and four
arguments, and every host layer offers the calls."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "rrtx_obstacle_release_polygon_batch"
FLAGS = "rrtx_polygons_set_active"
ARGS = ["ctx", "obstacles", "k", "robot_radius", "delta", "r_min", "unblock", "offsets", "edge_ids", "cap", "needed"]
FLAG_ARGS = ["ctx", "obstacles", "k", "active"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_points():
    args = _prototype(NEW)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert args[0] == "rrtx_ctx *ctx" and args[1] == "const int32_t *obstacles" and args[2] == "int k"
    assert [args[i] for i in (3, 4, 5, 6)] == ["double robot_radius", "double delta", "double r_min", "int unblock"]
    assert [args[i] for i in (7, 8, 9, 10)] == ["int64_t *offsets", "int32_t *edge_ids", "int64_t cap", "int64_t *needed"]
    args = _prototype(FLAGS)
    assert args == ["rrtx_ctx *ctx", "const int32_t *obstacles", "int k", "const uint8_t *active"]
    # it sits directly below the appearing half: nothing but its own comment between the two prototypes
    h = _header()
    above = h.index("int rrtx_obstacle_sweep_polygon_batch(")
    here = h.index(f"int {NEW}(")
    between = h[h.index(";", above) + 1:here]
    assert here > above and re.sub(r"/\*.*?\*/", "", between, flags=re.S).strip() == ""
    comment = re.findall(r"/\*.*?\*/", h[:here], flags=re.S)[-1]
    for words in ("R/DRRT.jl:3048-3125", "R/DRRT.jl:3202-3290", ":3287", "RRTX_E_CAPACITY", "RRTX_E_INVALID", "RRTX_E_STATE",
                  "unblock != 0", "SUBSET", "delta"):
        assert words in comment, words
    stats = re.search(r"int64_t last_sweep_candidates;\s*/\*(.*?)\*/", h, flags=re.S)
    assert stats and NEW in stats.group(1)


def test_library_exports_them(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NEW) and hasattr(hip_lib, FLAGS)
    assert NEW in bound and len(bound[NEW]) == len(ARGS) == 11
    assert FLAGS in bound and len(bound[FLAGS]) == len(FLAG_ARGS) == 4
    assert bound[NEW] == bound["rrtx_obstacle_sweep_polygon_batch"]


def test_python_layers_offer_them():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    sig = inspect.signature(Context.obstacle_release_polygon_batch)
    assert list(sig.parameters) == ["self", "obstacles", "robot_radius", "delta", "r_min", "unblock", "cap"]
    assert sig.parameters["r_min"].default == 0.0 and sig.parameters["unblock"].default is False
    assert sig.parameters["cap"].default is None
    assert list(inspect.signature(Context.polygons_set_active).parameters) == ["self", "obstacles", "active"]
    sig = inspect.signature(drrt.obstacleReleasePolygonBatch)
    assert list(sig.parameters) == ["S", "KD", "obs", "unblock"] and sig.parameters["unblock"].default is False
    # the siblings keep their signatures
    sig = inspect.signature(Context.obstacle_sweep_polygon_batch)
    assert list(sig.parameters) == ["self", "obstacles", "robot_radius", "delta", "r_min", "block", "cap"]
    assert list(inspect.signature(Context.obstacle_release_batch).parameters) == ["self", "obstacles", "search_range",
                                                                                  "robot_radius", "unblock", "cap"]
    assert list(inspect.signature(drrt.obstacleSweepPolygonBatch).parameters) == ["S", "KD", "obs", "block"]
    assert list(inspect.signature(drrt.obstacleReleaseBatch).parameters) == ["S", "KD", "obs", "unblock"]


def test_julia_shim_and_documents_carry_them():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NEW}, LIBRRTX)" in jl and f"(:{FLAGS}, LIBRRTX)" in jl
    assert re.search(r"function obstacleReleaseBatch\(tree::HipTree, S::TS, obs::Vector\{Obstacle\}, unblock::Bool = false\)", jl)
    assert re.search(r"function obstacleReleaseBatch\(tree::HipTree, S::TS, obs::Vector\{SphereObstacle\}, unblock::Bool = false\)", jl)
    assert re.search(r"function setObstaclesUsed!\(tree::HipTree, S::TS, obs::Vector\{Obstacle\}, used::Bool\)", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert NEW in text and FLAGS in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *4\.16\b", design, flags=re.M)
    assert "is not part of this call" not in design
