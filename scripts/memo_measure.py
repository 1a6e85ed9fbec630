#!/usr/bin/env python3
"""What the memory of aligned queries (xm_context_set_memo) costs and saves, on bench.py's workload: 1,000,000 synthetic 150 bp single-end
reads against the 5 Mb synthetic reference, one context, the batch resident in HBM (xm_align_resident: every kernel + the copy of the streams to the host).

  (a) a batch nothing of which was seen: ms per call and kernel_ms with the memory off, and on with an empty memory (the overhead: collapse, lookup, insert)
  (b) the same batch again: all served
  (c) HBM bytes per remembered query
  (d) a batch in which 30 % of the queries were seen in the batch before

Every figure is the median of --repeats calls behind one unmeasured call of the same kind; one JSON line on stdout.

    python scripts/memo_measure.py [--reads 1000000] [--repeats 3] [--budget-mib 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mapper_amd import api, synth  # noqa: E402


def arrays(reads):
    n, length = len(reads), len(reads[0])
    return (np.ones(n, np.int32), np.stack([np.arange(n, dtype=np.int64) * length, np.zeros(n, np.int64)], axis=1).reshape(-1),
            np.stack([np.full(n, length, np.int32), np.zeros(n, np.int32)], axis=1).reshape(-1), np.concatenate(reads), np.zeros(n), np.ones(n))


def call(ctx, params):
    t = time.perf_counter()
    r = ctx.align_resident(params)
    return {"ms": (time.perf_counter() - t) * 1e3, "kernel_ms": r.kernel_ms, "launches": r.kernel_launches, "remembered": r.remembered, "copies": r.copies, "aligned": r.counters[0]}


def median(runs):
    out = {k: statistics.median(r[k] for r in runs) for k in ("ms", "kernel_ms")}
    out.update({k: runs[-1][k] for k in ("launches", "remembered", "copies", "aligned")})
    out["ms_all"] = [round(r["ms"], 3) for r in runs]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--ref-len", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget-mib", type=int, default=1024)
    a = ap.parse_args()
    params = api.AlignmentParameters()
    ref = synth.synthetic_reference(a.ref_len, seed=0xEC011)
    db = api.ReferenceDatabase([("syn", ref)])
    x = synth.synthetic_single_end(ref, a.reads, seed=0x5EED0001)[0]
    fresh = synth.synthetic_single_end(ref, a.reads - a.reads * 3 // 10, seed=0x5EED0077)[0]
    rng = np.random.default_rng(0x3E)
    y = [x[int(k)] for k in rng.choice(a.reads, a.reads * 3 // 10, replace=False)] + list(fresh)
    y = [y[int(k)] for k in rng.permutation(len(y))]
    ctx = db.new_context()
    budget = a.budget_mib << 20
    out = {"reads": a.reads, "ref_len": a.ref_len, "repeats": a.repeats, "budget_bytes": budget}

    ctx.upload_arrays(*arrays(x))
    call(ctx, params)
    out["a_off"] = median([call(ctx, params) for _ in range(a.repeats)])
    unseen, again = [], []
    for k in range(a.repeats + 1):  # (the memory is made anew for every repeat: an unseen batch is unseen once)
        ctx.set_memo(budget)
        first, second = call(ctx, params), call(ctx, params)
        if k:
            unseen.append(first)
            again.append(second)
    out["a_on_unseen"] = median(unseen)
    out["b_again_all_served"] = median(again)
    info = ctx.memo_info()
    out["c_memory"] = dict(info, bytes_per_query=round(info["bytes_used"] / max(1, info["entries"]), 1))

    ctx.set_memo(0)
    ctx.upload_arrays(*arrays(y))
    call(ctx, params)
    out["d_off"] = median([call(ctx, params) for _ in range(a.repeats)])
    thirty = []
    for k in range(a.repeats + 1):
        ctx.set_memo(budget)
        ctx.upload_arrays(*arrays(x))
        call(ctx, params)
        ctx.upload_arrays(*arrays(y))
        r = call(ctx, params)
        if k:
            thirty.append(r)
    out["d_on_30_percent_seen"] = median(thirty)
    ctx.close()
    db.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
