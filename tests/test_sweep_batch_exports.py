"""CPU-side checks of the batched sweep's boundary: include/rrtx.h declares the entry point, the library exports it,
the Python binding carries it with the header's ten arguments, and every host layer offers the call."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "rrtx_obstacle_sweep_batch"
ARGS = ["ctx", "obstacles", "k", "search_range", "robot_radius", "block", "offsets", "edge_ids", "cap", "needed"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{NEW}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NEW
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert args[1] == "const int32_t *obstacles" and args[3] == "const double *search_range" and args[6] == "int64_t *offsets"
    # the normative text sits above the prototype and cites the reference
    comment = re.findall(r"/\*.*?\*/", _header()[:_header().index(f"int {NEW}(")], flags=re.S)[-1]
    for words in ("R/DRRT_Q.jl:3195-3290", "R/DRRT_Q.jl:1777", "RRTX_E_CAPACITY", "RRTX_E_INVALID", "RRTX_E_STATE", "block != 0"):
        assert words in comment, words


def test_library_exports_it(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NEW)
    assert NEW in bound and len(bound[NEW]) == len(ARGS) == 10


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    assert list(inspect.signature(Context.obstacle_sweep_batch).parameters) == ["self", "obstacles", "search_range",
                                                                                "robot_radius", "block", "cap"]
    sig = inspect.signature(drrt.obstacleSweepBatch)
    assert list(sig.parameters) == ["S", "KD", "obs", "block"] and sig.parameters["block"].default is False


def test_julia_shim_and_documents_carry_it():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NEW}, LIBRRTX)" in jl
    assert re.search(r"function obstacleSweepBatch\(", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert NEW in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.12\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
