#!/bin/bash
# Device code of two builds of xm_capi.o, symbol by symbol: the gfx950 code object of each is unbundled and disassembled (llvm-objdump -d), addresses and
# encodings dropped, and the instruction text of every kernel and out-of-line device function compared.  Runs on the CPU.  Exit status 0: equal for every symbol.
# usage: scripts/codeobj_diff.sh BEFORE/xm_capi.o AFTER/xm_capi.o
set -e
LL=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
for v in a b; do
  o=$1; [ $v = b ] && o=$2
  $LL/llvm-objcopy --dump-section .hip_fatbin=$T/$v.fatbin $o /dev/null
  $LL/clang-offload-bundler --unbundle --type=o --input=$T/$v.fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$T/$v.co
  # "0000000000001000 <symbol>:" opens a symbol; an instruction line is "\tmnemonic operands // address: encoding"
  $LL/llvm-objdump -d $T/$v.co | awk -v dir=$T/$v 'BEGIN { system("mkdir -p " dir) }
    /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); n++; file = dir "/" name; order[n] = name; next }
    file != "" && /^\t/ { sub(/[ \t]*\/\/.*$/, ""); print > file; count[name]++ }
    END { for (i = 1; i <= n; i++) print order[i], count[order[i]] > (dir ".symbols") }'
done
rc=0
while read name n; do
  if [ ! -f $T/b/$name ]; then echo "$name ($n instructions): missing after"; rc=1
  elif cmp -s $T/a/$name $T/b/$name; then echo "$name ($n instructions): equal"
  else echo "$name ($n instructions): DIFFERENT"; rc=1; fi
done < $T/a.symbols
while read name n; do [ -f $T/a/$name ] || { echo "$name ($n instructions): new"; rc=1; }; done < $T/b.symbols
rm -rf $T
exit $rc
