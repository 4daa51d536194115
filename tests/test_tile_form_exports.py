"""CPU-side checks of the tile kernel's two forms at the boundary: rrtx_last_tile_form is declared in include/rrtx.h,
bound in the Python binding and offered by Context, it is an entry point of its own and no option number, RRTX_OPT_TUNE
value 8 is the bit the library decodes as the looped form, and header and DESIGN.md describe both the same way."""
import ctypes as C
import os
import re

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rrtx_last_tile_form"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_bound_and_exported(hip_lib):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "rrtx.h"), flags=re.S)
    assert re.search(r"\bint\s+rrtx_last_tile_form\s*\(\s*rrtx_ctx \*ctx,\s*int \*form\s*\)\s*;", header)
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    assert bound[NAME] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    assert hasattr(hip_lib, NAME)
    from rrtqx_3d_amd.context import Context
    assert callable(Context.last_tile_form)


def test_it_is_no_option():
    """the form is a fact about the last call: no RRTX_OPT_* number in the header or the binding, no case for it in
    rrtx_get_option or rrtx_set_option"""
    assert "TILE_FORM" not in " ".join(re.findall(r"^#define\s+(\w+)", _read("include", "rrtx.h"), flags=re.M))
    assert not [n for n in dir(_capi) if "TILE_FORM" in n]
    src = _read("rrtqx_3d_amd", "csrc", "rrtx_capi.hip")
    for fn in ("int rrtx_get_option(", "int rrtx_set_option("):
        body = src[src.index(fn):]
        assert "tile_form" not in body[:body.index("\n}\n")]
    own = src[src.index("int rrtx_last_tile_form("):]
    assert "*form = ctx->last_tile_form;" in own[:own.index("\n}\n")]


def test_tune_bit_is_decoded_once():
    """value 8 = bit 3 = TuneBits::loop_form, between place_pass (value 4) and the fields from bit 8 on"""
    src = _read("rrtqx_3d_amd", "csrc", "rrtx_internal.hpp")
    body = src[src.index("struct TuneBits {"):src.index("// One launch site per kernel template")]
    fields = re.findall(r"^\s+(?:bool|int) (\w+);", body, flags=re.M)
    assert fields == ["xy_order", "whole_chunks", "place_pass", "loop_form", "kz_bins", "g3_side", "cell_shift"]
    init = re.search(r"return TuneBits\{(.*)\};", body).group(1)
    assert [s.strip() for s in init.split(",")][:4] == ["(t & 1) != 0", "(t & 2) != 0", "(t & 4) != 0", "(t & 8) != 0"]
    nn = _read("rrtqx_3d_amd", "csrc", "kernels_nn.hip")
    assert nn.count("tune.loop_form") == 1 and nn.count("last_tile_form =") == 1


def test_documents_carry_both():
    header = _read("include", "rrtx.h")
    design = _read("DESIGN.md")
    for text, where in ((header, "include/rrtx.h"), (design, "DESIGN.md")):
        flat = re.sub(r"[\s*]+", " ", text)
        assert NAME in text, where
        assert re.search(r"0 no tile kernel.*1 looped.*2 straight", flat), where
        assert re.search(r"RRTX_OPT_TUNE`?\s+value 8|[Vv]alue 8 \(bit 3\)", flat), where
    assert NAME in _read("profiles", "README.md")
