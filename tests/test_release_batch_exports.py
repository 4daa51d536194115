"""CPU-side checks of the batched release's boundary: include/rrtx.h declares rrtx_obstacle_release_batch and
rrtx_graph_edges_unblock, the library exports them, the Python binding carries them with the header's ten and three
arguments, and every host layer offers the calls."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "rrtx_obstacle_release_batch"
ARGS = ["ctx", "obstacles", "k", "search_range", "robot_radius", "unblock", "offsets", "edge_ids", "cap", "needed"]
UNBLOCK = "rrtx_graph_edges_unblock"
UNBLOCK_ARGS = ["ctx", "edge_ids", "n"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_points():
    args = _declared(NEW)
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert args[1] == "const int32_t *obstacles" and args[3] == "const double *search_range" and args[5] == "int unblock"
    assert args[6] == "int64_t *offsets" and args[7] == "int32_t *edge_ids" and args[9] == "int64_t *needed"
    args = _declared(UNBLOCK)
    assert [a.split()[-1].lstrip("*") for a in args] == UNBLOCK_ARGS
    assert args[1] == "const int32_t *edge_ids" and args[2] == "int64_t n"
    # the normative text sits above the prototype and cites the reference
    comment = re.findall(r"/\*.*?\*/", _header()[:_header().index(f"int {NEW}(")], flags=re.S)[-1]
    for words in ("R/DRRT_Q.jl:3295-3362", ":3302", ":3342", ":1777", "RRTX_E_CAPACITY", "RRTX_E_INVALID", "RRTX_E_STATE",
                  "unblock != 0"):
        assert words in comment, words
    # set_dist replaces the original, Inf included: said where set_dist is declared
    comment = re.findall(r"/\*.*?\*/", _header()[:_header().index("int rrtx_graph_edges_set_dist(")], flags=re.S)[-1]
    assert "distOriginal" in comment and "Inf included" in comment and UNBLOCK in comment


def test_library_exports_them(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NEW) and hasattr(hip_lib, UNBLOCK)
    assert NEW in bound and len(bound[NEW]) == len(ARGS) == 10
    assert UNBLOCK in bound and len(bound[UNBLOCK]) == len(UNBLOCK_ARGS) == 3


def test_python_layers_offer_them():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    assert list(inspect.signature(Context.obstacle_release_batch).parameters) == ["self", "obstacles", "search_range",
                                                                                  "robot_radius", "unblock", "cap"]
    assert inspect.signature(Context.obstacle_release_batch).parameters["unblock"].default is False
    assert list(inspect.signature(Context.graph_edges_unblock).parameters) == ["self", "edge_ids"]
    sig = inspect.signature(drrt.obstacleReleaseBatch)
    assert list(sig.parameters) == ["S", "KD", "obs", "unblock"] and sig.parameters["unblock"].default is False
    assert list(inspect.signature(drrt.unblockEdges).parameters) == ["KD", "ids"]


def test_julia_shim_and_documents_carry_them():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NEW}, LIBRRTX)" in jl and f"(:{UNBLOCK}, LIBRRTX)" in jl
    assert re.search(r"function obstacleReleaseBatch\(", jl) and re.search(r"function unblockEdges\(", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert NEW in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.13\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
