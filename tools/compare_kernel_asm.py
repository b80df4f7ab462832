#!/usr/bin/env python
"""Has a move of kernels between translation units left the device code alone?  

    python tools/compare_kernel_asm.py OLD_CSRC NEW_CSRC --moved adjgrad.hip=adjgrad.hip,adjgrad_sage.hip --same lora.hip

Compiles the named files of both source directories to gfx950 assembly (``hipcc --cuda-device-only -S`` with the Makefile's
flags; files with per-file flags take them through ``--flags``), cuts every kernel from its ``.globl`` line to
``.end_amdhsa_kernel``, drops comments, replaces the function index in local labels and the kernel's own mangled name, and
compares the bodies line for line, kernel descriptor included.  ``--moved OLD=NEW1,NEW2``: every kernel of OLD must appear in
exactly one of the NEW files; ``--same F``: the same file on both sides; ``--renamed OLD=NEW``: the kernel printed as OLD (as in
the report: demangled, no namespaces, no argument list) is looked up under the name NEW (respelled template parameters).

Verdicts: ``identical``; ``reordered`` -- the same multiset of opcodes and the same ``.amdhsa_*`` descriptor lines, in another
order or with other register names (a hand-written loop exchanged for an inlined helper); ``different`` -- the
opcode counts differ, but matrix, LDS, memory and barrier instruction counts are equal, registers and LDS bytes are not above
the old kernel's and neither side uses scratch; ``DIFFERENT`` -- anything else.  The last two carry the opcode-count
differences.  Prints one JSON document -- per old file and kernel ``[result, compared lines, file that holds it now, details]``
-- and exits 1 unless every verdict is ``identical`` or named by ``--accept``."""
import argparse
import collections
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


def opcodes(body):
    """Multiset of the opcodes of a normalised body (labels and directives left out)."""
    count = collections.Counter()
    for t in body:
        if not t.startswith(".") and not t.endswith(":"):
            count[t.split()[0]] += 1
    return count


def descriptor(body):
    return sorted(t for t in body if t.startswith(".amdhsa_"))


def field(body, name):
    return next(int(t.split()[1], 0) for t in body if t.split()[0] == ".amdhsa_" + name)


CLASSES = {"v_mfma": r"v_mfma", "ds": r"ds_", "memory loads": r"(global|buffer|flat)_load", "memory stores": r"(global|buffer|flat)_store",
           "s_barrier": r"s_barrier$"}


def difference(old, new):
    """What a kernel that differs has to meet: equal counts of matrix, LDS, memory and barrier instructions,
    registers (VGPR + AGPR, one file on gfx950) and LDS bytes not above the old kernel's, no scratch on either side."""
    co, cn = opcodes(old), opcodes(new)
    rec = {"opcode_counts_old_new": {k: [co[k], cn[k]] for k in sorted(set(co) | set(cn)) if co[k] != cn[k]}}
    within = True
    for label, pat in CLASSES.items():
        n_old = sum(v for k, v in co.items() if re.match(pat, k))
        n_new = sum(v for k, v in cn.items() if re.match(pat, k))
        rec[label] = [n_old, n_new]
        within &= n_old == n_new
    for label, name in (("registers", "next_free_vgpr"), ("lds_bytes", "group_segment_fixed_size"),
                        ("scratch_bytes", "private_segment_fixed_size")):
        rec[label] = [field(old, name), field(new, name)]
    within &= rec["registers"][1] <= rec["registers"][0] and rec["lds_bytes"][1] <= rec["lds_bytes"][0]
    within &= rec["scratch_bytes"] == [0, 0]
    rec["within_conditions"] = bool(within)
    return rec


def verdict(old, new):
    if old == new:
        return "identical", None
    if opcodes(old) == opcodes(new) and descriptor(old) == descriptor(new):
        return "reordered", None
    d = difference(old, new)
    return ("different" if d["within_conditions"] else "DIFFERENT"), d


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
    ap.add_argument("--accept", action="append", default=[], choices=["reordered", "different"],
                    help="verdicts besides `identical` that leave the exit status 0")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    extra = {f.split("=", 1)[0]: f.split("=", 1)[1].split(",") for f in a.flags}
    filt = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/usr/bin/c++filt") if os.path.exists(p)), None)
    plan = [(m.split("=", 1)[0], m.split("=", 1)[1].split(",")) for m in a.moved] + [(f, [f]) for f in a.same]
    renamed = dict(r.split("=", 1) for r in a.renamed)
    accept = {"identical", *a.accept}
    cache = {}

    def compiled(side, csrc, name):
        if (side, name) not in cache:
            cache[side, name] = kernels(csrc, name, extra.get(name, []), a.hipcc)
        return cache[side, name]

    report, ok, total, claimed = {}, True, 0, set()
    for old_name, new_names in plan:
        old = compiled("old", a.old, old_name)
        new = {n: compiled("new", a.new, n) for n in new_names}
        entry = report[old_name] = {}
        by_short = {short(s, filt): s for n in new_names for s in new[n]}
        now = lambda sym: by_short.get(renamed.get(short(sym, filt)), sym)
        for sym, body in sorted(old.items()):
            holders = [n for n in new_names if now(sym) in new[n]]
            detail = None
            if len(holders) != 1:
                result, where = ("missing" if not holders else "duplicated"), holders
            else:
                where = holders[0]
                claimed.add((where, now(sym)))
                result, detail = verdict(body, new[where][now(sym)])
            ok &= result in accept
            total += 1
            entry[short(sym, filt)] = [result, len(body), where] + ([detail] if detail else [])
    added = sorted(f"{n}: {short(s, filt)}" for (side, n), ks in cache.items() if side == "new" for s in ks if (n, s) not in claimed)
    if added:
        ok = False
    print(json.dumps({"kernels": total, "all_accepted": ok, "accepted": sorted(accept), "files": report,
                      "kernels the old files do not have": added}, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
