"""rrtx_extend_closest_self_dubins through every layer that can be checked without a GPU: the header's prototypes and
contract, the library's exports, the binding table, the Context / drrt signatures, the Julia shim and the documents."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi, drrt
from rrtqx_3d_amd.context import Context
from test_julia_shim_signatures import c_class, header_protos, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV = "rrtx_extend_closest_self_dubins", "rrtx_extend_closest_self_dubins_dev"
ARGS = ["ctx", "q", "nq", "k", "robot_radius", "r_min", "skip", "want", "tree_idx", "idx", "key", "cost_out", "cost_in",
        "word_out", "word_in", "hit_out", "hit_in", "count", "tree_cost_out", "tree_cost_in", "tree_word_out", "tree_word_in",
        "tree_hit_out", "tree_hit_in"]
CLASSES = ["ptr", "ptr", "i32", "i32", "f64", "f64"] + ["ptr"] * 18


def _text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_prototypes():
    protos = header_protos()
    for name in (HOST, DEV):
        assert name in protos, name
        ret, args = protos[name]
        assert ret == "int"
        assert [a.split()[-1].lstrip("*") for a in args] == ARGS
        assert [c_class(a) for a in args] == CLASSES
        assert args[1].startswith("const double")
        assert all(args[i].startswith(t) for i, t in ((6, "const uint8_t"), (7, "const uint8_t"), (8, "const int32_t")))
        assert all(args[i].startswith("double") for i in (10, 11, 12, 18, 19))
    text = _text("include", "rrtx.h")
    # the host form behind rrtx_extend_candidates_self_dubins, the device form behind its device form
    order = [text.index(f"int {n}(") for n in ("rrtx_extend_closest_self", "rrtx_extend_candidates_self_dubins", HOST,
                                                 "rrtx_extend_candidates_self_dubins_dev", DEV, "rrtx_pack_hits_dev")]
    assert order == sorted(order)
    assert text.index(f"int {HOST}(") < text.index("device-resident variants") < text.index(f"int {DEV}(")
    assert len(re.findall(r"^#define RRTX_CLOSEST_SELF_MAX_K 32$", text, flags=re.M)) == 1
    assert not re.search(r"RRTX_OPT_\w*CLOSEST", text)                 # no new option


def test_header_comment_states_the_contract():
    text = _text("include", "rrtx.h")
    at = text.index(f"int {HOST}(")
    comment = " ".join(text[text.rindex("/* ----", 0, at):at].replace("\n *", " ").split())
    for word in ("closestNode", "R/DRRT_Q.jl:1930-1935", "dim == 4", "rrtx_set_wrap", "RRTX_CLOSEST_SELF_MAX_K",
                 "RRTX_E_STATE", "RRTX_E_INVALID", "all NULL or all given", "may be NULL", "polygon list",
                 "an empty tree is fine", "all four coordinates are finite", "skip[j] == 0", "2^w copies",
                 "rrtx_extend_candidates_self_dubins", "p + period", "p - period", "NO copy is skipped", "taken as it is",
                 "min over all 2^w slots", "unfused", "want[j] != 0", "i < j", "(s, i)", "count[j]", "idx = -1", "+Inf",
                 "three zero bytes", "still a candidate", "q_j -> q_i", "q_i -> q_j", "WHOLE",
                 "RRTX_OPT_SPACE_HAS_TIME", "!validMove", "rrtx_set_dubins_velocity", "RRTX_OPT_DUBINS_TIME_COLUMN",
                 "moving polygons", "active flags", "rrtx_dubins_edges_check", "rrtx_nodes_count", "not an error",
                 "nearest_idx", "first entry whose sample was inserted", "key < nearest_dist[j]", "lower index", "exhausted",
                 "k-th key is not below", "kdFindNearest", "[0, period]", "monotone", "inside the period",
                 "outside the period", "Exact, no tolerance"):
        assert word.lower() in comment.lower(), word
    dev_at = text.index(f"int {DEV}(")
    dev_comment = text[text.rindex("/*", 0, dev_at):dev_at]
    assert "enqueues" in dev_comment and "bounded" in dev_comment and "once" in dev_comment
    # the SimpleEdge call keeps its scope and points here
    at = text.index("int rrtx_extend_closest_self(")
    simple = text[text.rindex("/* ----", 0, at):at]
    assert "out of scope" in simple and HOST in simple


def test_library_exports_and_binding(hip_lib):
    for name in (HOST, DEV):
        assert hasattr(hip_lib, name), name
        rows = [row for row in _capi.SYMBOLS if row[0] == name]
        assert len(rows) == 1 and len(rows[0][2]) == 24, name
        assert [c_class_of(t) for t in rows[0][2]] == CLASSES


def c_class_of(t):
    import ctypes as C
    return {C.c_int: "i32", C.c_double: "f64"}.get(t, "ptr")


def test_python_layers():
    sig = inspect.signature(Context.extend_closest_self_dubins)
    assert list(sig.parameters) == ["self", "q", "k", "robot_radius", "r_min", "skip", "want", "tree_idx"]
    assert all(sig.parameters[p].default is None for p in ("skip", "want", "tree_idx"))
    p = list(inspect.signature(Context.extend_closest_self_dubins_dev).parameters)
    assert len(p) == 24 and p[0] == "self" and p[1:6] == ["q_ptr", "nq", "k", "robot_radius", "r_min"]
    assert p[-2:] == ["tree_hit_out_ptr", "tree_hit_in_ptr"]
    p = inspect.signature(drrt.extend_closest_self_dubins).parameters
    assert list(p) == ["tree", "S", "newPositions", "k", "skip", "want", "treeNearest"]
    assert all(p[n].default is None for n in ("skip", "want", "treeNearest"))
    src = inspect.getsource(drrt.extend_closest_self_dubins)
    assert "_dubins_space(" in src and "S.robotRadius" in src and "S.minTurningRadius" in src


def test_julia_shim():
    calls = [c for c in julia_ccalls() if c[0] == HOST]
    assert len(calls) == 1
    txt = _text("julia", "RRTXHip.jl")
    m = re.search(r"function extend_closest_self_dubins\(tree::HipTree, S::TS, positions::Array\{Float64,2\}, k::Int;\s*skip", txt)
    assert m, "extend_closest_self_dubins(tree, S, positions, k; skip = nothing, want = nothing, treeNearest = nothing)"
    assert "S.robotRadius, S.minTurningRadius" in txt[m.start():m.start() + 4000]


def test_documents():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "extend_closest_self_dubins" in _text(doc), doc
    design = _text("DESIGN.md")
    assert re.search(r"^### 4\.20 ", design, flags=re.M)
    section = design[design.index("### 4.20 "):]
    for word in ("closest_rows4_kernel", "closest_fill4_kernel", "closest_plan4_kernel", "self_table4_kernel", "[0, period]",
                 "VGPR", "LDS", "scratch", "tools/time_extend_closest_dubins.py"):
        assert word in section, word
    # the open item the call answers is struck from the list
    open_items = design[design.index("Batched extend, open"):]
    assert "the closestNode rule in the Dubins spaces" not in open_items
