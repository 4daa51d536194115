"""CPU-side checks of the selection step's boundary: include/rrtx.h declares the new entry points, the library
exports them, and the RRTX_SEL_* / option values the Python binding carries are the header's."""
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rrtx_extend_select_dev", "rrtx_extend_select", "rrtx_node_cost_set")


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_header_declares_the_selection_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name


def test_library_exports_them(hip_lib):
    bound = {n for n, _, _ in _capi.SYMBOLS}
    for name in NEW:
        assert hasattr(hip_lib, name), name
        assert name in bound, name


def test_status_codes_match_the_header():
    defs = dict(re.findall(r"#define\s+(RRTX_(?:SEL|OPT)_[A-Z_]+)\s+(-?\d+)", _header()))
    sel = {k: int(v) for k, v in defs.items() if k.startswith("RRTX_SEL_")}
    assert sorted(sel) == ["RRTX_SEL_EMPTY", "RRTX_SEL_NO_PARENT", "RRTX_SEL_OK", "RRTX_SEL_OVERFLOW", "RRTX_SEL_UNSAFE"]
    assert len(set(sel.values())) == len(sel) and all(0 <= v < 256 for v in sel.values())
    for name, value in sel.items():
        assert getattr(_capi, name) == value, name
    assert _capi.RRTX_OPT_SELECT_LIST_CAP == int(defs["RRTX_OPT_SELECT_LIST_CAP"])


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    for m in ("node_cost_set", "extend_select", "extend_select_dev", "select_out_buffers"):
        assert callable(getattr(Context, m)), m
    assert callable(drrt.extend_select)
