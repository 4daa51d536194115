"""rrtx_extend_closest_self through every layer that can be checked without a GPU: the header's prototypes and contract,
the library's exports, the binding table, the Context / drrt signatures, the Julia shim and the documents."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi, drrt
from rrtqx_3d_amd.context import Context
from test_julia_shim_signatures import c_class, header_protos, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV = "rrtx_extend_closest_self", "rrtx_extend_closest_self_dev"
ARGS = ["ctx", "q", "nq", "k", "robot_radius", "skip", "want", "tree_idx", "idx", "cost", "hit_out", "hit_in", "count",
        "tree_hit_out", "tree_hit_in"]
CLASSES = ["ptr", "ptr", "i32", "i32", "f64"] + ["ptr"] * 10


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_prototypes():
    protos = header_protos()
    for name in (HOST, DEV):
        assert name in protos, name
        ret, args = protos[name]
        assert ret == "int"
        assert [a.split()[-1].lstrip("*") for a in args] == ARGS
        assert [c_class(a) for a in args] == CLASSES
        assert args[1].startswith("const double")
        assert all(args[i].startswith(t) for i, t in ((5, "const uint8_t"), (6, "const uint8_t"), (7, "const int32_t")))
    text = _header()
    assert re.search(r"^#define RRTX_CLOSEST_SELF_MAX_K 32$", text, flags=re.M)
    # next to the extend calls: the host form behind rrtx_extend_candidates_self, the device form among the device forms
    order = [text.index(f"int {n}(") for n in ("rrtx_extend_candidates_self", HOST, "rrtx_extend_candidates_dubins",
                                                 "rrtx_extend_candidates_self_dev", DEV,
                                                 "rrtx_extend_candidates_dubins_dev")]
    assert order == sorted(order)
    assert text.index(f"int {HOST}(") < text.index("device-resident variants") < text.index(f"int {DEV}(")


def test_header_comment_states_the_contract():
    text = _header()
    at = text.index(f"int {HOST}(")
    comment = " ".join(text[text.rindex("/* ----", 0, at):at].replace("\n *", " ").split())
    for word in ("closestNode", "R/DRRT_Q.jl:1930-1935", "i < j", "(s, i)", "skip", "want", "sample_unsafe", "count[j]",
                 "idx = -1", "+Inf", "RRTX_OPT_EXTEND_OBSTACLES", "RRTX_E_STATE", "RRTX_E_INVALID", "WHOLE",
                 "rrtx_edges_check", "rrtx_nodes_count", "not an error", "an empty tree is fine", "out of scope",
                 "rrtx_extend_candidates_self_dubins", "exhausted", "nearest_dist", "lower index", "Exact, no tolerance"):
        assert word.lower() in comment.lower(), word
    dev_at = text.index(f"int {DEV}(")
    dev_comment = text[text.rindex("/*", 0, dev_at):dev_at]
    assert "enqueues" in dev_comment and "bounded" in dev_comment


def test_library_exports_and_binding(hip_lib):
    for name in (HOST, DEV):
        assert hasattr(hip_lib, name), name
        rows = [row for row in _capi.SYMBOLS if row[0] == name]
        assert len(rows) == 1 and len(rows[0][2]) == 15, name
    assert _capi.RRTX_CLOSEST_SELF_MAX_K == 32


def test_python_layers():
    sig = inspect.signature(Context.extend_closest_self)
    assert list(sig.parameters) == ["self", "q", "k", "robot_radius", "skip", "want", "tree_idx"]
    assert all(sig.parameters[p].default is None for p in ("skip", "want", "tree_idx"))
    p = list(inspect.signature(Context.extend_closest_self_dev).parameters)
    assert len(p) == 15 and p[0] == "self" and p[-2:] == ["tree_hit_out_ptr", "tree_hit_in_ptr"]
    p = inspect.signature(drrt.extend_closest_self).parameters
    assert list(p) == ["tree", "S", "newPositions", "k", "skip", "want", "treeNearest"]
    assert all(p[n].default is None for n in ("skip", "want", "treeNearest"))


def test_julia_shim():
    assert HOST in {c[0] for c in julia_ccalls()}
    txt = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    m = re.search(r"function extend_closest_self\(tree::HipTree, S::TS, positions::Array\{Float64,2\}, k::Int;\s*skip", txt)
    assert m, "extend_closest_self(tree, S, positions, k; skip = nothing, want = nothing, treeNearest = nothing)"


def test_documents():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "extend_closest_self" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4\.19 ", design, flags=re.M)
    assert "closest_rows_kernel" in design
    # the open item the call answers is struck from the list, and the integration guide no longer leaves the search to
    # the caller
    assert "still needs the one-sample path" not in design
    assert "is the caller's to find" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
