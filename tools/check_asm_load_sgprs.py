#!/usr/bin/env python3
"""Reads hipcc's assembly of csrc/paths_fused.hip (``--save-temps`` with the Makefile's flags: ``*-gfx950.s``) and lists every
buffer load whose descriptor SGPRs were written by a vector-ALU instruction (v_readlane / v_readfirstlane: a spilled
descriptor coming back) fewer than five wait states earlier.  The product waves' loads are assembly statements, which hipcc's
hazard pass does not look into; a load that follows such a reload too closely reads the descriptor's OLD words (bload4's
comment in paths_fused.hip).  Exit status 1 if any is found.

    python tools/check_asm_load_sgprs.py paths_fused-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import re
import sys


def scan(path):
    lines = open(path).read().split("\n")
    kernel, found = None, []
    for i, line in enumerate(lines):
        m = re.match(r"(_Z\S+):", line)
        if m:
            kernel = m.group(1)
        m = re.match(r"\s*buffer_load_dword(?:x[234])?\s+\S+,\s*\S+,\s*s\[(\d+):(\d+)\]", line)
        if not m:
            continue
        lo, hi = int(m.group(1)), int(m.group(2))
        states, j = 0, i - 1
        while j > 0 and states < 5:
            t = lines[j].strip()
            j -= 1
            if not t or t.startswith((";", ".")):
                continue
            if t.startswith("s_nop"):
                states += int(t.split()[1]) + 1
                continue
            states += 1
            w = re.match(r"v_read(?:first)?lane_b32\s+s(\d+),", t)
            if w and lo <= int(w.group(1)) <= hi and states <= 5:
                found.append((kernel, i + 1, states, t, line.strip()))
    return found


if __name__ == "__main__":
    bad = [f for p in sys.argv[1:] for f in scan(p)]
    for kernel, ln, states, write, load in bad:
        print(f"{kernel}: line {ln}: `{write}` {states} wait state(s) in front of `{load}`")
    print(f"{len(bad)} load(s) too close behind a reload of their descriptor")
    sys.exit(1 if bad else 0)
