"""CPU-side checks of the delta cost update's boundary: include/rrtx.h declares rrtx_graph_cost_update_delta with its
nine arguments, the library exports it, the Python binding carries it, and every host layer and document offers it."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "rrtx_graph_cost_update_delta"
ARGS = ["rrtx_ctx *ctx", "int root_idx", "int store", "int32_t *node", "double *lmc", "int32_t *parent_edge", "int64_t cap",
        "int64_t *needed", "int32_t *passes"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_point():
    assert _declared(NEW) == ARGS
    # declared next to rrtx_graph_cost_update, the normative text above the prototype cites the reference
    head = _header()
    assert head.index("int rrtx_graph_cost_update(") < head.index(f"int {NEW}(") < head.index("int rrtx_points_check(")
    comment = re.findall(r"/\*.*?\*/", head[:head.index(f"int {NEW}(")], flags=re.S)[-1]
    for words in ("R/DRRT_Q.jl:2647-2817", "RRTX_E_CAPACITY", "RRTX_E_INVALID", "store != 0", "rrtx_node_cost_set",
                  "rrtx_graph_edges_clear", "ascending", "+Inf / -1"):
        assert words in comment, words


def test_library_exports_it(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NEW)
    assert NEW in bound and len(bound[NEW]) == len(ARGS) == 9


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    sig = inspect.signature(Context.graph_cost_update_delta)
    assert list(sig.parameters) == ["self", "root_idx", "store", "cap"]
    assert sig.parameters["store"].default is False and sig.parameters["cap"].default is None
    sig = inspect.signature(drrt.costUpdateDelta)
    assert list(sig.parameters) == ["KD", "root", "store"] and sig.parameters["store"].default is False


def test_julia_shim_and_documents_carry_it():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NEW}, LIBRRTX)" in jl
    assert re.search(r"function costUpdateDelta\(", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert NEW in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.14\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
