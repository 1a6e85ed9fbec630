#!/bin/bash
# Device code of two builds of an object (xm_align_kernel.o, xm_capi.o, xm_index_device.o, ...), symbol by symbol: the gfx950 code object of each is unbundled and disassembled (llvm-objdump -d), addresses and
# encodings dropped, and the instruction text of every kernel and out-of-line device function compared.  Runs on the CPU.  Exit status 0: equal for every symbol.
# A displacement from the program counter to another symbol (s_getpc_b64, s_add_u32 with a literal) is compared as the symbol and offset it points at
# (scripts/codeobj_resolve.py): adding or resizing a kernel moves everything behind it, and with that every such literal, without changing an instruction.
# The s_nop 0 padding behind a symbol's last instruction is not compared either: it follows the address the function happens to start at.  Every other s_nop is.
# Nor is the "..." line llvm-objdump prints for the zero bytes that pad the last symbol of a section.
# With more than one AFTER object (a unit that was split), a symbol of BEFORE is looked up in the union of them; one found in two of them is an error.
# usage: scripts/codeobj_diff.sh BEFORE/xm_align_kernel.o AFTER/xm_align_kernel.o [AFTER/another.o ...]   (any objects with a gfx950 bundle)
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
LL=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
[ $# -ge 2 ] || { echo "usage: $0 BEFORE.o AFTER.o [AFTER.o ...]" >&2; exit 2; }
nb=$(($# - 1))
for k in $(seq 0 $nb); do
  v=b$k; [ $k = 0 ] && v=a
  o=$1; shift
  $LL/llvm-objcopy --dump-section .hip_fatbin=$T/$v.fatbin $o /dev/null
  $LL/clang-offload-bundler --unbundle --type=o --input=$T/$v.fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/$v.co
  # "0000000000001000 <symbol>:" opens a symbol; an instruction line is "\tmnemonic operands // address: encoding"
  $LL/llvm-objdump -t $T/$v.co > $T/$v.symtab
  $LL/llvm-objdump -d $T/$v.co | python3 $HERE/codeobj_resolve.py $T/$v.symtab | awk -v dir=$T/$v 'BEGIN { system("mkdir -p " dir) }
  # (the instructions of a symbol go to a numbered file: the mangled names of library kernels are longer than a file name may be)
    /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); n++; if (file != "") close(file); file = dir "/" n; order[n] = name; next }
    file != "" && /^\t/ { sub(/[ \t]*\/\/.*$/, ""); print > file; count[n]++ }
    END { for (i = 1; i <= n; i++) print order[i], count[i] + 0, i > (dir ".symbols") }'
done
rc=0
declare -A after before
for k in $(seq 1 $nb); do
  while read name n i; do
    [ -z "${after[$name]}" ] || { echo "$name ($n instructions): in more than one object after"; rc=1; }
    after[$name]=b$k/$i
  done < $T/b$k.symbols
done
while read name n i; do
  before[$name]=$i
  j=${after[$name]}
  [ -f $T/a/$i ] || : > $T/a/$i
  [ -z "$j" ] || [ -f $T/$j ] || : > $T/$j
  if [ -z "$j" ]; then echo "$name ($n instructions): missing after"; rc=1
  elif cmp -s $T/a/$i $T/$j; then echo "$name ($n instructions): equal"
  else echo "$name ($n instructions): DIFFERENT"; rc=1; fi
done < $T/a.symbols
for k in $(seq 1 $nb); do
  while read name n i; do [ -n "${before[$name]}" ] || { echo "$name ($n instructions): new"; rc=1; }; done < $T/b$k.symbols
done
rm -rf $T
exit $rc
