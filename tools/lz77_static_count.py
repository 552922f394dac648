#!/usr/bin/env python3
"""Static instruction counts of a match-finder kernel, from hipcc's assembly (no GPU).

usage: hipcc -O3 -gline-tables-only -std=c++17 --offload-arch=gfx950 -Iinclude -Imoonbit-flate_amd/csrc \
             --cuda-device-only -S moonbit-flate_amd/csrc/lz77_kernels.hip -o lz77.s
       tools/lz77_static_count.py lz77.s <substring of the mangled kernel name> moonbit-flate_amd/csrc/lz77_kernels.hip

Prints (a) every instruction between the kernel's label and its s_endpgm, and (b) the instructions of the dense batch:
an instruction counts if the line table puts it on a line of lz77_stream between the progress guard's comment and the
sparse branch, or if it belongs to an inlined helper (another file, or a line above lz77_stream) and follows such an
instruction.  The kernel holds two inlined copies of the batch (interior and window edge), so (b) is their sum, rare
paths included; -gline-tables-only does not change the code (count (a) is the same without it)."""
import re
import sys

asm = open(sys.argv[1]).read().split("\n")
key = sys.argv[2]
src = open(sys.argv[3]).read().split("\n")


def line_of(text):
    return next(i + 1 for i, l in enumerate(src) if text in l)


lo, hi = line_of("// Progress guard: every batch moves the parser"), line_of("// =============================== sparse batch")
stream0 = line_of("FLATE_D void lz77_stream(")
# the line table's numbers of the source file itself (the compiler's version decides whether that is 0, 1 or both)
main = {int(m.group(1)) for m in (re.match(r'\s*\.file\s+(\d+)\s.*"([^"]*)"(\s+md5\s+\S+)?\s*$', l) for l in asm)
        if m and m.group(2).endswith(sys.argv[3].split("/")[-1])}
start = next(i for i, l in enumerate(asm) if l.startswith("_ZN") and key in l.split(":")[0])
end = next(i for i in range(start, len(asm)) if asm[i].strip().startswith("s_endpgm"))
cur, last, total, dense = (0, 0), "S", 0, 0
for l in asm[start + 1:end + 1]:
    t = l.strip()
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
    if m:
        cur = (int(m.group(1)), int(m.group(2)))
        continue
    if not t or t[0] in ";." or re.match(r"^(\.LBB\d+_\d+|\d+):", t):
        continue
    total += 1
    if cur[0] in main and cur[1] >= stream0:
        last = "D" if lo <= cur[1] < hi else "S"
    dense += last == "D"
print("%s: %d instructions, %d of them in the dense batch (both copies)" % (asm[start].split(":")[0], total, dense))
