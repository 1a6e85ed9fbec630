#!/usr/bin/env python3
"""Static account of the loads of launch-wide constants in the out-of-line device functions of the lane-per-read kernel (profiles/r13).

Input: the optimised device LLVM IR of xm_align_kernel.hip (hipcc <product flags> --offload-device-only -emit-llvm -S), and the byte offsets of the
members concerned (printed by a host program from offsetof; passed as KEY=VALUE).  For every function whose first argument is a ReadCtx& or whose
second is a SeedEnv const&, the loads are classified by the SSA value their address derives from:
  view-pointer   the load of ReadCtx::ix / SeedEnv::ix (or ::lc) itself: a private access of 8 bytes per lane
  view-field     a load through that pointer at a constant offset inside IndexView (generic address space: the kernel's frame copy, private memory)
  params-field   a load at a constant offset inside ReadCtx::params
  caps-field     a load at a constant offset inside ReadCtx::caps, or through SeedEnv::caps
  constant-as    a load whose address is in address space 4 (with a uniform address: a scalar load)
Addresses that pass through a phi or a select are not followed (none of the accesses in question does).  Output: a markdown table.
usage: uniform_loads.py dev.ll ix=0 caps=8 capsSize=84 params=160 paramsSize=80 seed=304 viewSize=168 [params=-1 when ReadCtx has none]"""
import re, sys

def main():
    ll = sys.argv[1]
    o = dict((k, int(v)) for k, v in (a.split("=") for a in sys.argv[2:]))
    fn = None
    rows = []
    for line in open(ll):
        m = re.match(r"define .* @(\S+?)\((.*)", line)
        if m:
            name = m.group(1)
            cx = se = None
            # the mangled parameter list: R NS_7ReadCtxE first -> %0 is the context; RKNS_7SeedEnvE second -> %1 is the seed environment
            if re.search(r"ERNS_7ReadCtxE", name): cx = "%0"
            if re.search(r"E(RNS_4CompE|RNS_12PathsCounterE)RKNS_7SeedEnvE", name): se = "%1"
            fn = dict(name=name, cx=cx, se=se, off={}, cls={}, cnt=dict.fromkeys(("view-pointer", "view-field", "params-field", "caps-field", "constant-as", "loads"), 0))
            if cx: fn["off"][cx] = ("cx", 0)
            if se: fn["off"][se] = ("se", 0)
            continue
        if fn is None: continue
        if line.startswith("}"):
            if fn["cx"] or fn["se"] or "xm_align_kernel" in fn["name"]: rows.append(fn)
            fn = None
            continue
        m = re.match(r"\s+(%\S+) = getelementptr (?:inbounds )?(?:nuw )?(?:nusw )?i8, ptr(?: addrspace\(\d\))? (%\S+), i64 (-?\d+)\s*$", line)
        if m and m.group(2) in fn["off"]:
            base, k = fn["off"][m.group(2)]
            fn["off"][m.group(1)] = (base, k + int(m.group(3)))
            continue
        m = re.match(r"\s+(%\S+) = load (.+?), ptr( addrspace\(\d\))? (%\S+?),", line)
        if not m: continue
        fn["cnt"]["loads"] += 1
        dst, ty, asp, ptr = m.groups()
        if asp and "(4)" in asp:
            fn["cnt"]["constant-as"] += 1
            continue
        if ptr not in fn["off"]: continue
        base, k = fn["off"][ptr]
        if base == "cx":
            if k == o["ix"] or k == o["seed"]:
                if ty.startswith("ptr"): fn["cnt"]["view-pointer"] += 1; fn["off"][dst] = ("view", 0)
            elif o.get("params", -1) >= 0 and o["params"] <= k < o["params"] + o["paramsSize"]: fn["cnt"]["params-field"] += 1
            elif o["caps"] <= k < o["caps"] + o["capsSize"]: fn["cnt"]["caps-field"] += 1
        elif base == "se":
            if k == 0 and ty.startswith("ptr"): fn["cnt"]["view-pointer"] += 1; fn["off"][dst] = ("view", 0)
            elif k == 8 and ty.startswith("ptr"): fn["off"][dst] = ("capsp", 0)
        elif base == "view" and 0 <= k < o["viewSize"]: fn["cnt"]["view-field"] += 1
        elif base == "capsp" and 0 <= k < o["capsSize"]: fn["cnt"]["caps-field"] += 1
    cols = ("loads", "view-pointer", "view-field", "params-field", "caps-field", "constant-as")
    print("| function | " + " | ".join(cols) + " |")
    print("|---|" + "---:|" * len(cols))
    tot = dict.fromkeys(cols, 0)
    import subprocess
    for fn in rows:
        nm = subprocess.run(["c++filt", fn["name"]], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "").split("(")[0]
        print("| `%s` | " % nm + " | ".join(str(fn["cnt"][c]) for c in cols) + " |")
        for c in cols: tot[c] += fn["cnt"][c]
    print("| **all listed** | " + " | ".join(str(tot[c]) for c in cols) + " |")

main()
