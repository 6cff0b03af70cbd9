#!/usr/bin/env python3
"""Fail the build when a kernel that must not spill uses scratch: check_spills.py REMARKS KERNEL...  REMARKS holds the compiler's
-Rpass-analysis=kernel-resource-usage output of one object, each KERNEL is a substring of the (mangled) names meant; the Makefile's
table says which files and kernels are held to the rule (gconv.hip and wgrad.hip for their hand-counted waits)."""
import re
import sys

if len(sys.argv) < 3:
    print("usage: check_spills.py REMARKS KERNEL...", file=sys.stderr)
    sys.exit(2)
text = open(sys.argv[1]).read()
wanted = sys.argv[2:]
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
print(f"check_spills: {seen} {'/'.join(wanted)} kernels, no scratch")
