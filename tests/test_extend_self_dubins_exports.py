"""rrtx_extend_candidates_self_dubins through every layer that can be checked without a GPU: the header's prototypes
and contract, the library's exports, the binding table, the Context / drrt signatures, the Julia shim and the documents."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi, drrt
from rrtqx_3d_amd.context import Context
from test_julia_shim_signatures import c_class, header_protos, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV = "rrtx_extend_candidates_self_dubins", "rrtx_extend_candidates_self_dubins_dev"
ARGS = ["ctx", "q", "nq", "r", "robot_radius", "r_min", "skip", "offsets", "idx", "key", "cost_out", "cost_in", "word_out",
        "word_in", "hit_out", "hit_in", "cap"]
CLASSES = ["ptr", "ptr", "i32", "f64", "f64", "f64"] + ["ptr"] * 10 + ["i64", "ptr"]


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
        assert args[1].startswith("const double") and args[6].startswith("const uint8_t")
    # the host form follows rrtx_extend_candidates_dubins and comes before the device-resident block, the device form
    # follows rrtx_extend_candidates_dubins_dev
    text = _header()
    order = [text.index(f"int {n}(") for n in ("rrtx_extend_candidates", "rrtx_extend_candidates_self",
                                                 "rrtx_extend_candidates_dubins", HOST, "rrtx_nn_nearest_dev",
                                                 "rrtx_extend_candidates_dev", "rrtx_extend_candidates_self_dev",
                                                 "rrtx_extend_candidates_dubins_dev", DEV)]
    assert order == sorted(order)
    assert text.index(f"int {HOST}(") < text.index("device-resident variants") < text.index(f"int {DEV}(")


def test_header_comment_states_the_contract():
    text = _header()
    at = text.index(f"int {HOST}(")
    start = text.rindex("/* ----", 0, at)
    comment = " ".join(text[start:at].replace("\n *", " ").split())          # (a phrase may run over a line break)
    for word in ("i < j", "skip", "RRTX_E_CAPACITY", "RRTX_E_STATE", "R/kdTree_general.jl:830", "R/ghostPoint.jl", "first_ge",
                 "first_gt", "least significant bit", "period / 2", "LOWEST", "sample_unsafe", "non-finite", "no root rule",
                 "ascending", "The tree is not read", "RRTX_OPT_SPACE_HAS_TIME", "rrtx_set_dubins_velocity",
                 "RRTX_OPT_DUBINS_TIME_COLUMN", "may be NULL", "radius per sample is out of scope"):
        assert word.lower() in comment.lower(), word
    dev_at = text.index(f"int {DEV}(")
    dev_comment = text[text.rindex("/*", 0, dev_at):dev_at]
    assert "needed_dev" in dev_comment and "at or beyond cap" in dev_comment and "enqueues" in dev_comment
    # the 3-D call's comment points here and keeps the radius per sample out of scope
    at3 = text.index("int rrtx_extend_candidates_self(")
    comment3 = " ".join(text[text.rindex("/* ----", 0, at3):at3].replace("\n *", " ").split())
    assert HOST in comment3 and "radius per sample is out of scope" in comment3
    assert "Dubins lists and a radius per sample" not in comment3


def test_library_exports_and_binding(hip_lib):
    for name in (HOST, DEV):
        assert hasattr(hip_lib, name), name
        rows = [row for row in _capi.SYMBOLS if row[0] == name]
        assert len(rows) == 1 and len(rows[0][2]) == 18, name


def test_python_layers():
    sig = inspect.signature(Context.extend_candidates_self_dubins)
    assert list(sig.parameters) == ["self", "q", "r", "robot_radius", "r_min", "skip", "cap"]
    assert sig.parameters["skip"].default is None and sig.parameters["cap"].default is None
    p = list(inspect.signature(Context.extend_candidates_self_dubins_dev).parameters)
    assert len(p) == 18 and p[0] == "self" and p[6] == "skip_ptr" and p[-1] == "needed_ptr"
    p = inspect.signature(drrt.extend_candidates_self_dubins).parameters
    assert list(p) == ["tree", "S", "newPositions", "hyberBallRad_", "skip"] and p["skip"].default is None
    p = inspect.signature(drrt.extend_candidates_dubins).parameters
    assert list(p) == ["tree", "S", "newPositions", "hyberBallRad_"]
    for fn in (drrt.extend_candidates_self_dubins, drrt.extend_candidates_dubins):
        src = inspect.getsource(fn)
        assert "S.minTurningRadius" in src and "S.robotRadius" in src


def test_julia_shim():
    calls = {c[0]: c for c in julia_ccalls()}
    assert HOST in calls and len(calls[HOST][2]) == 18
    txt = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    m = re.search(r"function extend_candidates_self_dubins\(tree::HipTree, S::TS, positions::Array\{Float64,2\}, "
                  r"hyberBallRad::Float64;\s*skip", txt)
    assert m, "extend_candidates_self_dubins(tree, S, positions, r; skip = nothing)"


def test_documents():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "extend_candidates_self_dubins" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^### 4\.18 ", design, flags=re.M)
    section = design[re.search(r"^### 4\.18 ", design, flags=re.M).start():]
    for word in ("self_join4_kernel", "self_table4_kernel", "VGPR", "launch_candidate_dubins"):
        assert word in section, word
