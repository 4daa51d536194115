"""CPU-side checks of RRTX_OPT_DUBINS_TIME_COLUMN's boundary: the option and its two values carry the same numbers in
include/rrtx.h, the Python binding and the Julia shim, every host layer offers it, and the library exports nothing new
for it -- the feature is an option, not an entry point."""
import os
import re
import subprocess

from rrtqx_3d_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("RRTX_OPT_DUBINS_TIME_COLUMN", "RRTX_TIME_COLUMN_PIECEWISE", "RRTX_TIME_COLUMN_RUNNING_SUM")


def _header():
    return open(os.path.join(ROOT, "include", "rrtx.h")).read()


def test_numbers_agree_in_header_python_and_julia():
    defs = dict(re.findall(r"^#define\s+(RRTX_[A-Z_]+)\s+(-?\d+)\s*$", _header(), flags=re.M))
    jl = open(os.path.join(ROOT, "julia", "RRTXHip.jl")).read()
    for name in NAMES:
        assert name in defs, name
        assert getattr(_capi, name) == int(defs[name]), name
        m = re.search(rf"^const {name} = \w+\((-?\d+)\)", jl, flags=re.M)
        assert m and int(m.group(1)) == int(defs[name]), name
    assert (int(defs[NAMES[1]]), int(defs[NAMES[2]])) == (0, 1)
    # the next free option number: no other option has it
    opts = {k: int(v) for k, v in defs.items() if k.startswith("RRTX_OPT_")}
    n = opts.pop(NAMES[0])
    assert n == max(opts.values()) + 1 and n not in opts.values()
    assert re.search(r"RRTX_OPT_DUBINS_TIME_COLUMN, Int64\(value\)", jl) and "function setDubinsTimeColumn(" in jl


def test_library_exports_nothing_new(hip_lib):
    """What the library exports is what the header declares (plus the measuring hooks of the clocks build, absent
    here), and none of it is about the time column."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rrtx_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" [TW] rrtx_", line)}
    assert exported == declared
    assert not [s for s in exported if "time_column" in s or "running" in s]
    assert sorted(n for n, _, _ in _capi.SYMBOLS) == sorted(declared)


def test_python_layers_offer_it():
    from rrtqx_3d_amd import drrt
    from rrtqx_3d_amd.context import Context
    assert callable(Context.set_dubins_time_column) and isinstance(Context.dubins_time_column, property)
    S = drrt.CSpace(4, 0.1, [0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 1])
    assert S.dubinsTimeColumn == _capi.RRTX_TIME_COLUMN_PIECEWISE


def test_documents_carry_it():
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "RRTX_OPT_DUBINS_TIME_COLUMN" in open(os.path.join(ROOT, doc)).read(), doc
