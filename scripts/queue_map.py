#!/usr/bin/env python3
"""Which hardware queue every stream of a bench.py run dispatched to, and what the contexts did between their align kernels.

usage: queue_map.py DIR > queue_map.json
DIR holds the csv output of `rocprofv3 --kernel-trace --hip-trace --output-format csv -- python bench.py` (…_kernel_trace.csv, …_hip_api_trace.csv).

A stream is a (Stream_Id, Queue_Id) pair, written "stream/queue": a HIP stream dispatches to one hardware queue, and the trace's Stream_Id alone is not unique (the traces of
profiles/r07 carry one id for two streams that live on different queues and are driven by different host threads).  A context is a stream that ran xm_align_kernel.  The timed region starts when every context has finished its first call (the warm-up: a call ends with
xm_gather_kernel) and ends with the last dispatch of a context.  Times are milliseconds."""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict


def find(d, suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    return hits[0] if hits else None


def short(name):
    m = re.search(r"(xm\w*_kernel|__amd_rocclr_\w+)", name)
    return m.group(1) if m else name[:60]


def overlap(a, b):
    """total time two sorted lists of (start, end) intervals run side by side"""
    i = j = 0
    t = 0
    while i < len(a) and j < len(b):
        lo, hi = max(a[i][0], b[j][0]), min(a[i][1], b[j][1])
        if hi > lo:
            t += hi - lo
        if a[i][1] < b[j][1]:
            i += 1
        else:
            j += 1
    return t


def main(d):
    rows = []
    with open(find(d, "kernel_trace.csv"), newline="") as f:
        reader = csv.DictReader(f)
        missing = [c for c in ("Queue_Id", "Stream_Id", "Thread_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp") if c not in (reader.fieldnames or [])]
        if missing:
            sys.exit("queue_map.py: the kernel trace has no column " + ", ".join(missing))
        for r in reader:
            rows.append({"q": int(r["Queue_Id"]), "s": "%d/%d" % (int(r["Stream_Id"]), int(r["Queue_Id"])), "tid": int(r["Thread_Id"]), "k": short(r["Kernel_Name"]),
                         "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])})
    rows.sort(key=lambda r: r["t0"])
    ms = lambda ns: round(ns / 1e6, 3)
    streams = defaultdict(list)
    for r in rows:
        streams[r["s"]].append(r)
    ctx_streams = sorted(s for s, v in streams.items() if any(r["k"] == "xm_align_kernel" for r in v))
    if not ctx_streams:
        sys.exit("queue_map.py: no xm_align_kernel dispatch in the trace")
    first_done = [next((r["t1"] for r in streams[s] if r["k"] == "xm_gather_kernel"), streams[s][0]["t0"]) for s in ctx_streams]
    w0 = max(first_done)
    w1 = max(r["t1"] for s in ctx_streams for r in streams[s])
    out = {"queues_with_dispatches": sorted({r["q"] for r in rows}), "timed_region_ms": ms(w1 - w0), "streams": {}, "contexts": {}}
    for s, v in sorted(streams.items()):
        by = defaultdict(int)
        for r in v:
            by[r["k"]] += 1
        out["streams"][str(s)] = {"queues": sorted({r["q"] for r in v}), "host_threads": sorted({r["tid"] for r in v}), "dispatches": len(v),
                                  "dispatches_in_timed_region": sum(1 for r in v if r["t0"] >= w0), "by_kernel": dict(sorted(by.items(), key=lambda kv: -kv[1])[:8])}
    align = {}
    for s in ctx_streams:
        v = [r for r in streams[s] if r["t0"] >= w0]
        al = [(r["t0"], r["t1"]) for r in v if r["k"] == "xm_align_kernel"]
        align[s] = al
        other = defaultdict(lambda: [0, 0, 0])
        for r in v:
            if r["k"] != "xm_align_kernel":
                o = other[r["k"]]
                o[0] += 1; o[1] += r["t1"] - r["t0"]; o[2] = max(o[2], r["t1"] - r["t0"])
        # between the end of one dispatch of the stream and the start of the next: nothing of this context is on the GPU (host turn-around, copies by DMA, waiting for a queue)
        idle = sum(max(0, b["t0"] - a["t1"]) for a, b in zip(v, v[1:]))
        # hand-over between two align kernels of one call: what lies between them
        hand = [(a, b) for a, b in zip(al, al[1:]) if not any(r["k"] == "xm_gather_kernel" and a[1] <= r["t0"] <= b[0] for r in v)]
        hand_disp = sum(1 for a, b in hand for r in v if a[1] <= r["t0"] < b[0] and r["k"] != "xm_align_kernel")
        out["contexts"][str(s)] = {"queues_of_align_kernels": sorted({r["q"] for r in v if r["k"] == "xm_align_kernel"}), "align_launches": len(al),
                                   "align_ms": ms(sum(b - a for a, b in al)), "stream_idle_ms": ms(idle),
                                   "pass_hand_overs": len(hand), "pass_hand_over_ms": ms(sum(b[0] - a[1] for a, b in hand)), "compute_dispatches_in_hand_overs": hand_disp,
                                   "other_dispatches": {k: {"n": o[0], "ms": ms(o[1]), "max_ms": ms(o[2])} for k, o in sorted(other.items(), key=lambda kv: -kv[1][1])}}
    out["align_overlap_ms"] = {"%s+%s" % (a, b): ms(overlap(align[a], align[b])) for i, a in enumerate(ctx_streams) for b in ctx_streams[i + 1:]}
    out["contexts_sharing_a_queue"] = [[a, b] for i, a in enumerate(ctx_streams) for b in ctx_streams[i + 1:]
                                       if set(out["contexts"][str(a)]["queues_of_align_kernels"]) & set(out["contexts"][str(b)]["queues_of_align_kernels"])]
    api = find(d, "hip_api_trace.csv")
    if api:
        ctx_threads = {r["tid"] for s in ctx_streams for r in streams[s] if r["t0"] >= w0}
        calls = defaultdict(lambda: defaultdict(lambda: [0, 0, 0]))
        allocs = defaultdict(int)
        with open(api, newline="") as f:
            for r in csv.DictReader(f):
                t0, t1, tid, fn = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Thread_Id"]), r["Function"]
                if t0 < w0 or t0 > w1:
                    continue
                if fn in ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamCreate", "hipStreamCreateWithFlags", "hipStreamDestroy"):
                    allocs[fn] += 1
                if tid in ctx_threads:
                    c = calls[tid][fn]
                    c[0] += 1; c[1] += t1 - t0; c[2] = max(c[2], t1 - t0)
        out["allocation_calls_in_timed_region"] = dict(allocs)
        out["host_threads"] = {str(t): {fn: {"n": c[0], "ms": ms(c[1]), "max_ms": ms(c[2])} for fn, c in sorted(v.items(), key=lambda kv: -kv[1][1])[:6]} for t, v in calls.items()}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main(sys.argv[1])
