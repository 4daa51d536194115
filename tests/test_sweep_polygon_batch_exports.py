"""CPU-side checks of the batched polygon sweep's boundary: include/rrtx.h declares the entry point, the library exports
it, the Python binding carries it with the header's eleven arguments, and every host layer offers the call."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "rrtx_obstacle_sweep_polygon_batch"
ARGS = ["ctx", "obstacles", "k", "robot_radius", "delta", "r_min", "block", "offsets", "edge_ids", "cap", "needed"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{NEW}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NEW
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert args[1] == "const int32_t *obstacles" and args[7] == "int64_t *offsets" and args[8] == "int32_t *edge_ids"
    assert [args[i] for i in (3, 4, 5, 6)] == ["double robot_radius", "double delta", "double r_min", "int block"]
    # it sits below the single call, and the normative text above the prototype cites the reference
    assert _header().index(f"int {NEW}(") > _header().index("int rrtx_obstacle_sweep_polygon(")
    comment = re.findall(r"/\*.*?\*/", _header()[:_header().index(f"int {NEW}(")], flags=re.S)[-1]
    for words in ("R/DRRT.jl:3048-3125", "R/DRRT.jl:3127-3200", "RRTX_E_CAPACITY", "RRTX_E_INVALID", "RRTX_E_STATE", "block != 0"):
        assert words in comment, words
    stats = re.search(r"int64_t last_sweep_candidates;\s*/\*(.*?)\*/", _header(), flags=re.S)
    assert stats and NEW in stats.group(1)


def test_library_exports_it(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NEW)
    assert NEW in bound and len(bound[NEW]) == len(ARGS) == 11


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    sig = inspect.signature(Context.obstacle_sweep_polygon_batch)
    assert list(sig.parameters) == ["self", "obstacles", "robot_radius", "delta", "r_min", "block", "cap"]
    assert sig.parameters["r_min"].default == 0.0 and sig.parameters["block"].default is False
    assert sig.parameters["cap"].default is None
    sig = inspect.signature(drrt.obstacleSweepPolygonBatch)
    assert list(sig.parameters) == ["S", "KD", "obs", "block"] and sig.parameters["block"].default is False
    # the sphere batch keeps its signature
    assert list(inspect.signature(drrt.obstacleSweepBatch).parameters) == ["S", "KD", "obs", "block"]


def test_julia_shim_and_documents_carry_it():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NEW}, LIBRRTX)" in jl
    assert re.search(r"function obstacleSweepBatch\(tree::HipTree, S::TS, obs::Vector\{Obstacle\}, block::Bool = false\)", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert NEW in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.15\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
