#!/usr/bin/env python3
"""Fail the build when a gconv / wgrad kernel of conv.hip uses scratch (see the Makefile rule for conv.o).  Further arguments
name other kernels to hold to the same rule: substrings of their (mangled) names, as for metrics.o."""
import re
import sys

text = open(sys.argv[1]).read()
wanted = sys.argv[2:] or ["gconv_kernel", "gconv_pkernel", "wgrad_kernel"]
bad, seen = [], 0
for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S):
    name, scratch = m.group(1), int(m.group(2))
    if any(w in name for w in wanted):
        seen += 1
        if scratch:
            bad.append((name, scratch))
for line in text.splitlines():
    if "warning:" in line or "error:" in line:
        print(line)
if bad or not seen:
    for name, scratch in bad:
        print(f"SPILL: {name}: {scratch} bytes/lane of scratch", file=sys.stderr)
    if not seen:
        print("check_spills: no %s kernel found in the resource remarks" % "/".join(wanted), file=sys.stderr)
    sys.exit(1)
print(f"check_spills: {seen} {'MFMA' if len(sys.argv) < 3 else '/'.join(wanted)} kernels, no scratch")
