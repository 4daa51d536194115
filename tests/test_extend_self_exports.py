"""rrtx_extend_candidates_self through every layer that can be checked without a GPU: the header's prototypes and
contract, the library's exports, the binding table, the Context / drrt signatures, the Julia shim and the documents."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi, drrt
from rrtqx_3d_amd.context import Context
from test_julia_shim_signatures import c_class, header_protos, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV = "rrtx_extend_candidates_self", "rrtx_extend_candidates_self_dev"
ARGS = ["ctx", "q", "nq", "r", "robot_radius", "skip", "offsets", "idx", "cost", "hit_out", "hit_in", "cap"]
CLASSES = ["ptr", "ptr", "i32", "f64", "f64", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "i64", "ptr"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_prototypes():
    protos = header_protos()
    for name, last in ((HOST, "needed"), (DEV, "needed_dev")):
        assert name in protos, name
        ret, args = protos[name]
        assert ret == "int"
        assert [a.split()[-1].lstrip("*") for a in args] == ARGS + [last]
        assert [c_class(a) for a in args] == CLASSES
        assert args[1].startswith("const double") and args[5].startswith("const uint8_t")
    # the device form follows rrtx_extend_candidates_dev, the host form rrtx_extend_candidates: next to the extend calls,
    # and not between the two polygon-burst prototypes
    text = _header()
    order = [text.index(f"int {n}(") for n in ("rrtx_extend_candidates", HOST, "rrtx_extend_candidates_dubins",
                                                 "rrtx_extend_candidates_dev", DEV, "rrtx_extend_candidates_dubins_dev")]
    assert order == sorted(order)
    a, b = text.index("int rrtx_obstacle_sweep_polygon_batch("), text.index("int rrtx_obstacle_release_polygon_batch(")
    assert not any(min(a, b) < text.index(f"int {n}(") < max(a, b) for n in (HOST, DEV))


def test_header_comment_states_the_contract():
    text = _header()
    at = text.index(f"int {HOST}(")
    start = text.rindex("/* ----", 0, at)
    comment = " ".join(text[start:at].split())
    for word in ("i < j", "skip", "RRTX_E_CAPACITY", "R/kdTree_general.jl:830", "R/DRRT_Q.jl:1927-1979", "2581-2637",
                 "RRTX_OPT_EXTEND_OBSTACLES", "first_ge", "sample_unsafe", "non-finite", "no root rule", "ascending",
                 "The tree is not read", "out of scope"):
        assert word.lower() in comment.lower(), word
    dev_at = text.index(f"int {DEV}(")
    dev_comment = text[text.rindex("/*", 0, dev_at):dev_at]
    assert "needed_dev" in dev_comment and "at or beyond cap" in dev_comment and "enqueues" in dev_comment


def test_library_exports_and_binding(hip_lib):
    for name in (HOST, DEV):
        assert hasattr(hip_lib, name), name
        rows = [row for row in _capi.SYMBOLS if row[0] == name]
        assert len(rows) == 1 and len(rows[0][2]) == 13, name


def test_python_layers():
    p = list(inspect.signature(Context.extend_candidates_self).parameters)
    assert p == ["self", "q", "r", "robot_radius", "skip", "cap"]
    sig = inspect.signature(Context.extend_candidates_self)
    assert sig.parameters["skip"].default is None and sig.parameters["cap"].default is None
    p = list(inspect.signature(Context.extend_candidates_self_dev).parameters)
    assert len(p) == 13 and p[0] == "self" and p[-1] == "needed_ptr"
    p = inspect.signature(drrt.extend_candidates_self).parameters
    assert list(p) == ["tree", "S", "newPositions", "hyberBallRad_", "skip"] and p["skip"].default is None


def test_julia_shim():
    assert HOST in {c[0] for c in julia_ccalls()}
    txt = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    m = re.search(r"function extend_candidates_self\(tree::HipTree, S::TS, positions::Array\{Float64,2\}, "
                  r"hyberBallRad::Float64;\s*skip", txt)
    assert m, "extend_candidates_self(tree, S, positions, r; skip = nothing)"


def test_documents():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "extend_candidates_self" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4\.17 ", design, flags=re.M)
    assert "kernels_self.hip" in design
    # the caveat the new call answers is gone from the integration guide
    assert "do not see each other" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
