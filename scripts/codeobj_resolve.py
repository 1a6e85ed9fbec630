"""Filter of scripts/codeobj_diff.sh: llvm-objdump -d text of a gfx950 code object on stdin, its symbol table (llvm-objdump -t) as the argument.  The
literal of the s_add_u32 that follows an s_getpc_b64 is a displacement to another symbol (a device function, a constant table); it changes whenever
anything in front of either moves, e.g. when a kernel is added to the object.  It is replaced by what it points at, <symbol+offset>, so that two builds
compare equal exactly when the instructions and their targets are.  A run of "s_nop 0" behind the last instruction of a symbol is dropped for the same
reason: it is the padding up to the next symbol's alignment, never executed, and how long it is depends on the address the function starts at.  Every
s_nop that an instruction follows - the hazard nops, a loop head's padding - stays and is compared.  The "..." line the disassembler prints in place of
a run of zero bytes (the fill behind the last symbol of a section) is dropped too: it is not an instruction."""
import bisect
import re
import sys

syms = []
for line in open(sys.argv[1]):
    f = line.split()
    if len(f) >= 5 and re.fullmatch(r"[0-9a-f]{16}", f[0]) and "*ABS*" not in line and "*UND*" not in line and not f[-1].startswith("."):
        syms.append((int(f[0], 16), f[-1]))
syms.sort()
starts = [a for a, _ in syms]


def name_of(target):
    k = bisect.bisect_right(starts, target) - 1
    if k < 0:
        return "0x%x" % target
    return "<%s+0x%x>" % (syms[k][1], target - syms[k][0])


pc = None    # what the last s_getpc_b64 returns: the address of the instruction behind it
nops = []    # a run of "s_nop 0" lines whose end has not been seen yet

for line in sys.stdin:
    if line.strip() == "...":
        continue
    m = re.search(r"//\s*([0-9A-Fa-f]+):", line)
    if re.match(r"\ts_nop 0\s", line):
        nops.append(line)
        continue
    if m:  # an instruction follows the run: it is code
        sys.stdout.writelines(nops)
    del nops[:]
    if "s_getpc_b64" in line and m:
        pc = int(m.group(1), 16) + 4
    elif pc is not None:
        a = re.match(r"(\ts_add_u32 s\d+, s\d+, )0x([0-9a-f]+)(\s.*)$", line, re.S)
        if a:
            disp = int(a.group(2), 16)
            if disp >= 1 << 31:
                disp -= 1 << 32
            line = a.group(1) + name_of(pc + disp) + a.group(3)
        pc = None
    sys.stdout.write(line)
