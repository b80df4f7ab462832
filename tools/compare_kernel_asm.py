#!/usr/bin/env python
"""Has a move of kernels between translation units left the device code alone?  

    python tools/compare_kernel_asm.py OLD_CSRC NEW_CSRC --moved adjgrad.hip=adjgrad.hip,adjgrad_sage.hip --same lora.hip

Compiles the named files of both source directories to gfx950 assembly (``hipcc --cuda-device-only -S`` with the Makefile's
flags; files with per-file flags take them through ``--flags``), cuts every kernel from its ``.globl`` line to
``.end_amdhsa_kernel``, drops comments, replaces the function index in local labels and the kernel's own mangled name, and
compares the bodies line for line, kernel descriptor included.  ``--moved OLD=NEW1,NEW2``: every kernel of OLD must appear in
exactly one of the NEW files; ``--same F``: the same file on both sides; ``--renamed OLD=NEW``: the kernel printed as OLD (as in
the report: demangled, no namespaces, no argument list) is looked up under the name NEW (respelled template parameters).  Prints one JSON document -- per old file and kernel
``[result, compared lines, file that holds it now]`` -- and exits 1 unless everything is identical."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result -fvisibility=hidden -DLGNN_BUILDING".split()
LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)_(\d+)")
FUNC = re.compile(r"\.Lfunc_(begin|end)\d+")


def kernels(csrc, name, extra, hipcc):
    """{mangled kernel name: normalised body lines} of one source file."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([hipcc, *FLAGS, *extra, "--cuda-device-only", "-S", name, "-o", out], check=True, cwd=csrc)
        lines = open(out).read().split("\n")
    found = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        start = max(j for j in range(i) if re.match(r"\s*\.globl\s+" + re.escape(sym) + r"(\s|$)", lines[j]))
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = []
        for raw in lines[start:end + 1]:
            t = raw.split(";", 1)[0].strip()
            if t:
                body.append(FUNC.sub(r".Lfunc_\1", LABEL.sub(r".L\1_\3", t.replace(sym, "KERNEL"))))
        found[sym] = body
    return found


def short(sym, filt):
    if not filt:
        return sym
    d = subprocess.run([filt, sym], capture_output=True, text=True).stdout.strip()
    d = re.sub(r"^void ", "", d).replace("lgnn::", "").replace("(anonymous namespace)::", "")
    depth, cut = 0, len(d)
    for k, ch in enumerate(d):  # cut the argument list: the first '(' outside template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            cut = k
            break
    return d[:cut]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--moved", action="append", default=[], metavar="OLD=NEW1,NEW2")
    ap.add_argument("--same", action="append", default=[], metavar="FILE")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW", help="kernel names as the report prints them")
    ap.add_argument("--flags", action="append", default=[], metavar="FILE=FLAG,FLAG", help="per-file flags of the Makefile")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    extra = {f.split("=", 1)[0]: f.split("=", 1)[1].split(",") for f in a.flags}
    filt = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/usr/bin/c++filt") if os.path.exists(p)), None)
    plan = [(m.split("=", 1)[0], m.split("=", 1)[1].split(",")) for m in a.moved] + [(f, [f]) for f in a.same]
    renamed = dict(r.split("=", 1) for r in a.renamed)
    report, ok, total = {}, True, 0
    for old_name, new_names in plan:
        old = kernels(a.old, old_name, extra.get(old_name, []), a.hipcc)
        new = {n: kernels(a.new, n, extra.get(n, []), a.hipcc) for n in new_names}
        entry = report[old_name] = {}
        by_short = {short(s, filt): s for n in new_names for s in new[n]}
        now = lambda sym: by_short.get(renamed.get(short(sym, filt)), sym)
        for sym, body in sorted(old.items()):
            holders = [n for n in new_names if now(sym) in new[n]]
            if len(holders) != 1:
                result, where = ("missing" if not holders else "duplicated"), holders
            else:
                where = holders[0]
                result = "identical" if new[where][now(sym)] == body else "DIFFERENT"
            ok &= result == "identical"
            total += 1
            entry[short(sym, filt)] = [result, len(body), where]
        added = sorted(short(s, filt) for n in new_names for s in new[n] if s not in {now(o) for o in old})
        if added:
            ok = False
            entry["(kernels the old file does not have)"] = added
    print(json.dumps({"kernels": total, "all_identical": ok, "files": report}, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
