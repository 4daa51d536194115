"""CPU-side checks of the boundary of rrtx_extend_select_dubins: include/rrtx.h declares it, the library exports it,
_capi binds it with the header's argument count, and Context, drrt and the Julia shim carry it."""
import inspect
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rrtx_extend_select_dubins"
ARGS = ["rrtx_ctx *ctx", "const double *q", "int nq", "double r", "double robot_radius", "double r_min",
        "const double *lmc", "int32_t *parent_idx", "int64_t *parent_entry", "double *lmc_new", "uint8_t *status",
        "int64_t *rw_offsets", "int32_t *rw_node", "double *rw_value", "int64_t rw_cap", "int64_t *rw_needed",
        "int32_t *nearest_idx", "double *nearest_dist", "uint8_t *sample_unsafe", "int64_t *offsets", "int32_t *idx",
        "double *key", "double *cost_out", "double *cost_in", "uint8_t *hit_out", "uint8_t *hit_in", "int64_t cap",
        "int64_t *needed"]


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_header_declares_it():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{NAME}\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, NAME
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS


def test_header_comment_states_the_hold():
    head = _header()
    comment = re.findall(r"/\*.*?\*/", head[:head.index(f"int {NAME}(")], flags=re.S)[-1]
    comment = " ".join(comment.replace("\n *", " ").split())
    for words in ("dim == 4", "rrtx_extend_candidates_dubins_dev", "rrtx_extend_select_dev", "byte is zero",
                  "RRTX_OPT_SPACE_HAS_TIME", "RRTX_OPT_DUBINS_TIME_COLUMN", "rrtx_set_dubins_velocity", "RRTX_E_CAPACITY",
                  "three cost columns", "whether or not the nearest was asked for"):
        assert words in comment, words
    link = re.findall(r"/\*.*?\*/", head[:head.index("int rrtx_graph_edges_append_lists_dev(")], flags=re.S)[-1]
    assert NAME in link and "HOLD RULE" in link


def test_library_exports_it_and_capi_binds_it(hip_lib):
    bound = {n: a for n, _, a in _capi.SYMBOLS}
    assert hasattr(hip_lib, NAME)
    assert NAME in bound and len(bound[NAME]) == len(ARGS)


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    assert list(inspect.signature(Context.extend_select_dubins).parameters) == [
        "self", "q", "r", "robot_radius", "r_min", "lmc", "rw_cap", "out", "want_lists", "cap"]
    assert list(inspect.signature(drrt.extend_select_dubins).parameters)[:4] == ["tree", "S", "newPositions", "hyberBallRad_"]
    assert callable(drrt.registerSelectedEdges)


def test_julia_shim_and_documents_carry_it():
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    assert f"(:{NAME}, LIBRRTX)" in jl and re.search(r"\bfunction extend_select_dubins\(", jl)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md", os.path.join("profiles", "README.md")):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    assert re.search(r"^#+ *4\.22\b", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)
