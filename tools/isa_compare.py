#!/usr/bin/env python3
"""Compare the kernels of two sets of hipcc .s files instruction by instruction (comments, directives, symbol names and the
function numbers in block labels ignored) and by their resource metadata (VGPRs, SGPRs, AGPRs, LDS, scratch).
usage: isa_compare.py old.s new.s              -- one file each
       isa_compare.py old_dir new_dir          -- every *.s in each directory
       isa_compare.py old new REGEX=REPL ...   -- rename the old side's symbols first (re.sub), for a kernel whose name changed
Kernels are paired by symbol name; prints one line per kernel that differs, exists on one side only or appears in two files of one side,
then a summary line."""
import glob
import os
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    """{symbol: (instructions, {metadata key: value})} of one .s file"""
    code, name, body = {}, None, []
    lines = open(path).read().split("\n")
    for line in lines:
        if re.match(r"^_Z\S+:", line):
            name, body = line.split(":")[0], []
            continue
        if name is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end") or t.startswith(".end_amdhsa_kernel"):
            code[name] = body
            name = None
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        t = t.split(";")[0].strip()
        t = re.sub(r"_Z\w+", "SYM", t)
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)   # (block labels carry the function's position in its file)
        if t:
            body.append(t)
    # amdhsa.kernels metadata: one "  - " item per kernel, its own keys at four spaces of indentation
    meta, item = {}, None
    for line in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if line.startswith("  - "):
            item = {}
            line = "    " + line[4:]
        elif not line.startswith("    "):
            item = None
        if item is None or line.startswith("     "):
            continue
        key, _, val = line.strip().partition(":")
        if key == ".name":
            meta[val.strip()] = item
        elif key in META:
            item[key] = val.strip()
    return {k: (v, meta.get(k, {})) for k, v in code.items()}


def load(path):
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        for k, v in kernels(f).items():
            if k in out:   # (a kernel compiled into two units: only one copy is launched, and only one would be compared)
                print(f"TWICE IN {path}: {k} (again in {os.path.basename(f)})")
            out[k] = v
    return out


a, b = load(sys.argv[1]), load(sys.argv[2])
for pattern, _, repl in (arg.partition("=") for arg in sys.argv[3:]):
    a = {re.sub(pattern, repl, k): v for k, v in a.items()}
same = 0
for k in sorted(set(a) | set(b)):
    if k not in a or k not in b:
        print(f"ONLY IN {'new' if k in b else 'old'}: {k}")
        continue
    (ba, ma), (bb, mb) = a[k], b[k]
    if ba == bb and ma == mb:
        same += 1
        continue
    if ba != bb:
        first = next((i for i, (x, y) in enumerate(zip(ba, bb)) if x != y), min(len(ba), len(bb)))
        print(f"DIFF  {k}: {len(ba)} vs {len(bb)} instructions, first difference at {first}: "
              f"{ba[first] if first < len(ba) else None!r} vs {bb[first] if first < len(bb) else None!r}")
    if ma != mb:
        print(f"DIFF  {k}: metadata {ma} vs {mb}")
print(f"{len(a)} kernels vs {len(b)} kernels, {len(set(a) & set(b))} by name in both; {same} identical in instructions and "
      f"resources ({', '.join(m.lstrip('.') for m in META)})")
