"""CPU-side checks of the boundary of "the extend lists become mirror edges": include/rrtx.h declares the four entry
points, the library exports them, the Python binding, drrt and the Julia shim carry them, and the header's comment
states the order rule and the hold rule."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ["rrtx_ctx *ctx", "int nq", "const int64_t *offsets", "const int32_t *idx", "const double *cost_out",
         "const double *cost_in", "const uint8_t *hit_out", "const uint8_t *hit_in"]
TAIL = ["int64_t cap", "const int32_t *node_of", "int idx_is_batch", "int64_t *first_id", "int64_t *n_added",
        "int64_t *row_first"]
ARGS = {
    "rrtx_graph_edges_append_lists_dev": LISTS + ["const int64_t *n_valid_dev"] + TAIL,
    "rrtx_graph_edges_append_lists": LISTS + ["int64_t n_valid"] + TAIL,
    "rrtx_graph_edges_append_selected": ["rrtx_ctx *ctx", "int nq", "const int32_t *node_of", "int64_t *first_id",
                                         "int64_t *n_added", "int64_t *row_first"],
    "rrtx_graph_edges_get": ["rrtx_ctx *ctx", "const int32_t *ids", "int64_t first_id", "int64_t n", "int32_t *start",
                             "int32_t *end", "double *dist", "double *dist_original"],
}


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_four_entry_points():
    for name, args in ARGS.items():
        assert _declared(name) == args, name


def test_header_comment_names_the_order_rule_and_the_hold_rule():
    head = _header()
    comment = re.findall(r"/\*.*?\*/", head[:head.index("int rrtx_graph_edges_append_lists_dev(")], flags=re.S)[-1]
    comment = " ".join(comment.replace("\n *", " ").split())          # the comment's own line breaks
    for words in ("ORDER RULE", "for j = 0 .. nq-1", "in list order", "the out-edge v -> u, always", "hit_in[e] == 0",
                  "consecutive from rrtx_graph_edges_count", "HOLD RULE", "rrtx_nodes_append", "rrtx_node_cost_set",
                  "EVERY other entry point drops it", "RRTX_E_STATE", "RRTX_E_CAPACITY", "RRTX_E_INVALID",
                  "waits on the stream ONCE", "24 bytes", "rrtx_graph_edges_set_dist", "rrtx_graph_edges_block"):
        assert words in comment, words


def test_library_exports_them(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    for name, args in ARGS.items():
        assert hasattr(hip_lib, name), name
        assert name in bound and len(bound[name]) == len(args), name


def test_python_layers_offer_them():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    assert list(inspect.signature(Context.graph_edges_append_lists).parameters)[:9] == [
        "self", "offsets", "idx", "cost_out", "cost_in", "hit_out", "hit_in", "node_of", "idx_is_batch"]
    assert "node_of_ptr" in inspect.signature(Context.graph_edges_append_lists_dev).parameters
    assert list(inspect.signature(Context.graph_edges_append_selected).parameters)[:2] == ["self", "node_of"]
    assert list(inspect.signature(Context.graph_edges_get).parameters) == ["self", "ids", "first_id", "n"]
    for fn in ("registerEdgesFromLists", "registerSelectedEdges", "registeredEdges"):
        assert callable(getattr(drrt, fn)), fn


def test_julia_shim_and_documents_carry_them():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    for name in ARGS:
        assert f"(:{name}, LIBRRTX)" in jl, name
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "rrtx_graph_edges_append_selected" in text, doc
    assert re.search(r"^#+ *4\.21\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
