#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, function by function.

    python tools/device_code_diff.py OLD_OBJ_DIR NEW_OBJ_DIR

Both directories are csrc/_obj trees left by `python -m rrtqx_3d_amd.build --force --save-temps`.  Per source
(<name>-hip-amdgcn-amd-amdhsa-gfx950.s) the tool compares

  * every device function, instruction by instruction, with assembler comments dropped and the file-order numbers of
    local labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>, .LJTI<n>_) normalised,
  * the .amdhsa_kernel descriptor of every kernel,
  * the -Rpass-analysis=kernel-resource-usage block of every kernel (<name>.o.resource-usage.txt; the file:line prefix
    is ignored).

The __hip_cuid_<hash> symbol, a hash of the translation unit, lies outside of these and is not compared.  One line per
source, then ALL IDENTICAL or the list of what differs; a function or a source that exists on one side only is listed.
The exit status is 0 when everything is identical and 1 otherwise.  The tool compares text: it knows no instruction.
"""
from __future__ import annotations

import os
import re
import sys

ASM_SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_NUMBERED = re.compile(r"\.(LBB|LJTI)\d+_")
_ENDLABEL = re.compile(r"\.Lfunc_end\d+")
_TMP = re.compile(r"\.Ltmp(\d+)")
_REMARK = re.compile(r"^remark: \S+?:\d+:\d+: (.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]\s*$")


class Function:
    def __init__(self):
        self.lines = []        # normalised body: labels, directives and instructions in order
        self.descriptor = None  # lines of the .amdhsa_kernel block (kernels only)

    @property
    def instructions(self):
        return [l for l in self.lines if not l.startswith(".") and not l.endswith(":")]


def _normalise(line: str, tmps: dict) -> str:
    line = line.split(";", 1)[0].strip()
    line = re.sub(r"\s+", " ", line)
    line = _NUMBERED.sub(lambda m: "." + m.group(1) + "_", line)
    line = _ENDLABEL.sub(".Lfunc_end", line)
    return _TMP.sub(lambda m: ".Ltmp#%d" % tmps.setdefault(m.group(1), len(tmps)), line)


def parse_asm(text: str) -> dict:
    """{symbol: Function} of every function of one -gfx950.s file."""
    funcs, cur, name, tmps, desc = {}, None, None, {}, None
    pending = None   # a .type ...,@function line has named the symbol whose label comes next
    for raw in text.splitlines():
        if cur is None:
            m = _TYPE.match(raw)
            if m:
                pending = m.group(1)
            elif pending and raw.startswith(pending + ":"):
                cur, name, tmps, pending = Function(), pending, {}, None
            continue
        if desc is not None:                      # inside the kernel descriptor
            if raw.strip() == ".end_amdhsa_kernel":
                cur.descriptor, desc = desc, None
            else:
                desc.append(_normalise(raw, tmps))
            continue
        if _KERNEL.match(raw):
            desc = []
            continue
        if _FUNC_END.match(raw):
            funcs[name] = cur
            cur = None
            continue
        line = _normalise(raw, tmps)
        if line and not line.startswith(".section"):
            cur.lines.append(line)
    if cur is not None:
        funcs[name] = cur                         # (a truncated file: what there is of the last function)
    return funcs


def parse_resource_usage(text: str) -> dict:
    """{kernel symbol: the lines of its resource-usage block} of the compiler's remarks."""
    blocks, cur = {}, None
    for raw in text.splitlines():
        m = _REMARK.match(raw)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = blocks.setdefault(body.split(":", 1)[1].strip(), [])
        elif cur is not None:
            cur.append(body)
    return blocks


def compare_source(name, old_asm, new_asm, old_res="", new_res=""):
    """(summary line, list of differences) for one source; the texts of its two .s files and resource-usage files."""
    fo, fn = parse_asm(old_asm), parse_asm(new_asm)
    ro, rn = parse_resource_usage(old_res), parse_resource_usage(new_res)
    diffs, same, differing, desc_diff, res_cmp, res_diff, n_instr = [], 0, 0, 0, 0, 0, 0
    for sym in sorted(set(fo) | set(fn)):
        if sym not in fo or sym not in fn:
            diffs.append("%s: %s exists only in the %s" % (name, sym, "parent" if sym in fo else "branch"))
            differing += 1
            continue
        a, b = fo[sym], fn[sym]
        n_instr += len(b.instructions)
        if a.lines == b.lines:
            same += 1
        else:
            differing += 1
            at = next((i for i, (x, y) in enumerate(zip(a.lines, b.lines)) if x != y), min(len(a.lines), len(b.lines)))
            was = a.lines[at] if at < len(a.lines) else "<end>"
            now = b.lines[at] if at < len(b.lines) else "<end>"
            diffs.append("%s: %s differs at line %d of its body: `%s` -> `%s`" % (name, sym, at + 1, was, now))
        if a.descriptor != b.descriptor:
            desc_diff += 1
            diffs.append("%s: %s kernel descriptor differs" % (name, sym))
        if sym in ro or sym in rn:
            res_cmp += 1
            if ro.get(sym) != rn.get(sym):
                res_diff += 1
                diffs.append("%s: %s resource usage differs: %s -> %s" % (name, sym, ro.get(sym), rn.get(sym)))
    kernels = lambda f: sum(1 for x in f.values() if x.descriptor is not None)
    line = ("%s: %d kernels / %d device functions in parent, %d / %d in branch; %d identical, %d differing; "
            "kernel descriptors differing: %d; resource blocks compared: %d, differing: %d "
            "(%d lines; %d instruction lines compared)"
            % (name, kernels(fo), len(fo), kernels(fn), len(fn), same, differing, desc_diff, res_cmp, res_diff,
               len(new_asm.splitlines()), n_instr))
    return line, diffs


def _read(path: str) -> str:
    if not os.path.exists(path):
        return ""
    with open(path, errors="replace") as f:
        return f.read()


def compare_trees(old_dir: str, new_dir: str):
    """(summary lines, differences) over every source either tree has device assembly for."""
    names = lambda d: {f[: -len(ASM_SUFFIX)] for f in os.listdir(d) if f.endswith(ASM_SUFFIX)}
    old_names, new_names = names(old_dir), names(new_dir)
    lines, diffs = [], []
    for name in sorted(old_names | new_names):
        if name not in old_names or name not in new_names:
            diffs.append("%s: source exists only in the %s" % (name, "parent" if name in old_names else "branch"))
            continue
        line, d = compare_source(name, _read(os.path.join(old_dir, name + ASM_SUFFIX)),
                                 _read(os.path.join(new_dir, name + ASM_SUFFIX)),
                                 _read(os.path.join(old_dir, name + ".o.resource-usage.txt")),
                                 _read(os.path.join(new_dir, name + ".o.resource-usage.txt")))
        lines.append(line)
        diffs += d
    if not lines and not diffs:
        diffs.append("no *%s file in either tree" % ASM_SUFFIX)
    return lines, diffs


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__.strip().splitlines()[2].strip(), file=sys.stderr)
        return 2
    lines, diffs = compare_trees(argv[1], argv[2])
    print("\n".join(lines))
    if not diffs:
        print("ALL IDENTICAL")
        return 0
    print("DIFFERING:")
    print("\n".join("  " + d for d in diffs))
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
