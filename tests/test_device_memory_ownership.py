"""Who frees what is decided by types, not by a list: the four allocation calls of the HIP runtime appear in the owning
types of csrc/rrtx_internal.hpp (DevBuf, DevArray over it, PinnedBuf) and in no other file of csrc, and the context and
its cost-propagation state hold device and pinned memory through members of those types only -- so a workspace a later
change adds is released by its own destructor, whether or not anybody remembers it."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "rrtqx_3d_amd", "csrc")
OWNER = "rrtx_internal.hpp"
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")


def _code(text):
    """the text without // comments (a comment may name the calls)"""
    return "\n".join(line.split("//", 1)[0] for line in text.splitlines())


def _struct_body(text, name):
    """the members of `struct name { ... };` at the struct's own nesting depth (nested structs and function bodies cut)"""
    at = re.search(r"^struct\s+%s\s*\{" % name, text, re.M)
    assert at, name
    depth, out, i = 1, [], at.end()
    while depth > 0:
        c = text[i]
        if c == "{":
            depth += 1
        elif c == "}":
            depth -= 1
        elif depth == 1:
            out.append(c)
        i += 1
    return "".join(out)


def test_allocation_calls_live_in_the_owning_types_alone():
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp", ".h", ".cpp")):
            n = len(CALLS.findall(_code(open(os.path.join(CSRC, f)).read())))
            if n:
                found[f] = n
    assert list(found) == [OWNER], found


def test_context_and_graph_cost_hold_no_raw_pointer_to_device_or_pinned_memory():
    text = _code(open(os.path.join(CSRC, OWNER)).read())
    # a member declaration whose type ends in `*`: `double *nodes[4]`, `char *h_arena = nullptr`, `int32_t *a, *b` ...
    # (hipStream_t and hipEvent_t are handles; std::vector members, the registered ranges among them, start with std::)
    raw = re.compile(r"^\s*(?:const\s+)?(?:unsigned\s+)?[A-Za-z_][\w:]*(?:<[^;>]*>)?\s*\*+\s*\w+[^;()]*;", re.M)
    for name in ("rrtx_ctx", "GraphCost"):
        body = _struct_body(text, name)
        assert "DevBuf" in body, name                       # (the body was found: both structs hold buffers)
        members = [m.group(0).strip() for m in raw.finditer(body) if not m.group(0).lstrip().startswith("std::")]
        assert members == [], (name, members)


def test_owning_types_cannot_be_copied():
    """(the header asserts it where it is compiled; here: that the assertion is there and names every owning type)"""
    text = _code(open(os.path.join(CSRC, OWNER)).read())
    at = text.index("static_assert(!std::is_copy_constructible<DevBuf>::value")
    stmt = text[at:text.index(";", at)]
    assert "is_copy_constructible<DevArray<double>>" in stmt and "is_copy_constructible<PinnedBuf>" in stmt
