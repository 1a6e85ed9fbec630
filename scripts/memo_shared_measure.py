#!/usr/bin/env python3
"""One memory of aligned queries per GPU against one per context, on a stream with duplicates spread over the whole of it: --batches
batches of --reads synthetic 150 bp single-end reads against the 5 Mb synthetic reference (bench.py's configs[1] model) through --contexts contexts of one GPU
(multi.MultiGpuDatabase: batch k goes to context k mod N, the copy of the next batch overlaps the alignment of the current one).  A fraction --duplicates of
the stream's reads are copies of other reads of the stream, anywhere in it.

For every arrangement - no memory, one memory of --budget-mib / contexts per context, one shared two-generation memory of --budget-mib - one JSON line:
queries aligned (sum of counters[0]), served from a memory, served as copies within a batch, HBM the memories hold at the end, reads per second over the stream
(the spread over --repeats streams), and the host time the calls waited for the shared memory's mutex (xm_result.reserved: both critical sections).

    python scripts/memo_shared_measure.py [--reads 200000] [--batches 12] [--contexts 3] [--duplicates 0.1] [--budget-mib 3072] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mapper_amd import api, multi, synth  # noqa: E402


def arrays(reads):
    n, length = len(reads), len(reads[0])
    return (np.ones(n, np.int32), np.stack([np.arange(n, dtype=np.int64) * length, np.zeros(n, np.int64)], axis=1).reshape(-1),
            np.stack([np.full(n, length, np.int32), np.zeros(n, np.int32)], axis=1).reshape(-1), np.concatenate(reads), np.zeros(n), np.ones(n))


def stream_of(ref, total, duplicates, seed):
    """`total` reads of which a fraction `duplicates` are copies of others, in random order over the whole stream"""
    n_dup = int(total * duplicates)
    distinct = synth.synthetic_single_end(ref, total - n_dup, seed=seed)[0]
    rng = np.random.default_rng(seed + 1)
    picks = np.concatenate([np.arange(total - n_dup), rng.integers(total - n_dup, size=n_dup)])
    return [distinct[int(k)] for k in rng.permutation(picks)]


def one_stream(contigs, devices, warm, batches, params, **memo):
    db = multi.MultiGpuDatabase(contigs, devices, **memo)
    try:
        list(db.align_stream(iter(warm), params))  # (unmeasured, one batch of other reads per context: scratch and buffers)
        t = time.perf_counter()
        results = list(db.align_stream(iter(batches), params))
        seconds = time.perf_counter() - t
        held = sum(m.info()["bytes_used"] for m in db.memories) + sum(r.memo_info()["bytes_used"] for r in db.replicas)
        info = [m.info() for m in db.memories]
    finally:
        db.close()
    waits = [r.memory_wait_us for r in results]
    return {"seconds": seconds, "aligned": int(sum(r.counters[0] for r in results)), "remembered": int(sum(r.remembered for r in results)),
            "copies": int(sum(r.copies for r in results)), "hbm_bytes_held": int(held), "mutex_wait_us_per_call": {"median": float(np.median(waits)), "max": int(max(waits))},
            "memories": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--contexts", type=int, default=3)
    ap.add_argument("--duplicates", type=float, default=0.1)
    ap.add_argument("--ref-len", type=int, default=5_000_000)
    ap.add_argument("--budget-mib", type=int, default=3072)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    params = api.AlignmentParameters()
    ref = synth.synthetic_reference(a.ref_len, seed=0xEC011)
    contigs = [("syn", ref)]
    total = a.reads * a.batches
    stream = stream_of(ref, total, a.duplicates, 0x5EED0100)
    batches = [arrays(stream[k * a.reads:(k + 1) * a.reads]) for k in range(a.batches)]
    devices = [a.device] * a.contexts
    other = synth.synthetic_single_end(ref, a.reads * a.contexts, seed=0x5EED0200)[0]
    warm = [arrays(other[k * a.reads:(k + 1) * a.reads]) for k in range(a.contexts)]
    budget = a.budget_mib << 20
    for name, memo in (("none", {}), ("per_context", {"memo_bytes": budget // a.contexts}), ("shared", {"shared_memo_bytes": budget})):
        runs = [one_stream(contigs, devices, warm, batches, params, **memo) for _ in range(a.repeats)]
        rates = sorted(total / r["seconds"] / 1e6 for r in runs)
        out = {"arrangement": name, "reads": a.reads, "batches": a.batches, "contexts": a.contexts, "duplicates": a.duplicates, "budget_bytes": budget if memo else 0,
               "mreads_per_s": {"min": round(rates[0], 3), "median": round(float(np.median(rates)), 3), "max": round(rates[-1], 3)}}
        out.update({k: runs[-1][k] for k in ("aligned", "remembered", "copies", "hbm_bytes_held", "mutex_wait_us_per_call", "memories")})
        out["aligned_all_runs"] = [r["aligned"] for r in runs]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
