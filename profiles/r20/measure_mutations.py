"""Wall time of mutations(filter) by the host path (parent commit's module and this tree's) and by the device path, over two pile-ups on one GPU.

    python measure_mutations.py <reference bases> <reads> <repetitions> <tag>      (writes measure_<tag>.json beside this script)

parent_pileup.py, beside this script when it ran, is the parent commit's mapper_amd/pileup.py (git show <parent>:mapper_amd/pileup.py) with its two relative
imports made absolute; it is not kept here.  Both modules drive the same library."""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import oracle_lib
import parent_pileup
import pileup_workloads as W
from mapper_amd import api, multi, pileup, synth


def timed(f, reps):
    out, times = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        times.append(time.perf_counter() - t)
    return out, [round(x * 1000, 2) for x in times]


def main():
    ref_len, n_reads, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    tag = sys.argv[4]
    t0 = time.perf_counter()
    ref = synth.synthetic_reference(ref_len, seed=0xEC011)
    reads = synth.synthetic_single_end(ref[:min(ref_len, 5_000_000)], n_reads, seed=0x5EED0001, indel_prob=0.3)[0]
    half = len(reads) // 2
    batches = [oracle_lib.QueryBatch([W.single(r) for r in part]) for part in (reads[:half], reads[half:])]
    contigs = [("r", ref)]
    two = multi.MultiGpuDatabase(contigs, [0, 0])
    print("made reference, reads and index in %.1f s" % (time.perf_counter() - t0), flush=True)
    ms = {"parent": parent_pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True), "tree": pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True)}
    for rep, b in enumerate(batches):
        two.replicas[rep].align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())
        for m in ms.values():
            m.add_last(None, replica=rep)
    out = {"tag": tag, "reference": ref_len, "reads": n_reads, "replicas": 2, "events": len(ms["tree"]._events())}
    filters = {"default": pileup.MutationDetectionParameters.defaultFilter(), "loose": pileup.MutationDetectionParameters(2.0, 0.05, 1.0, 0.05, 1.0, 0.05)}
    for name, f in filters.items():
        pf = parent_pileup.MutationDetectionParameters(f.minSNPTotalDepth, f.minSNPDepthFraction, f.minIndelTotalStartDepth, f.minIndelStartDepthFraction,
                                                       f.minIndelContinuationTotalDepth, f.minIndelContinuationDepthFraction)
        # interleaved, host paths first (the device path moves the counts of the second pile-up into the first; the host path sums them either way)
        rows_parent, t_parent = timed(lambda: ms["parent"].mutations(pf), reps)
        rows_tree, t_tree = timed(lambda: ms["tree"].mutations(f), reps)
        rows_parent2, t_parent2 = timed(lambda: ms["parent"].mutations(pf), reps)
        rows_tree2, t_tree2 = timed(lambda: ms["tree"].mutations(f), reps)
        rows_gpu, t_gpu = timed(lambda: ms["tree"].mutations(f, on_gpu=True), reps + 2)
        figures = dict(ms["tree"].last_on_gpu)
        # the judge call alone (upload, kernel, verdicts down), as the device path makes it
        indels = list(ms["tree"]._indels().items())
        _, t_group = timed(lambda: ms["tree"]._indels(), 2)
        rows_after, t_after = timed(lambda: ms["tree"].mutations(f), 1)
        assert rows_parent == rows_tree == rows_gpu == rows_after == rows_parent2 == rows_tree2
        host_bytes = 48 * ref_len * 2
        out[name] = {"rows": len(rows_tree), "snp_rows": figures["snp_rows"], "candidates": len(indels), "host_parent_ms": t_parent + t_parent2, "host_tree_ms": t_tree + t_tree2,
                     "device_ms": t_gpu, "host_after_device_ms": t_after, "grouping_ms": t_group, "select_kernels_ms": round(figures["select_ms"], 3), "rows_d2h_ms": round(figures["d2h_ms"], 3),
                     "bytes_to_host_device_path": figures["bytes_to_host"], "bytes_to_host_host_path": host_bytes}
        print(json.dumps({name: out[name]}), flush=True)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure_%s.json" % tag), "w") as fh:
        json.dump(out, fh, indent=1)
    for m in ms.values():
        m.close()
    two.close()


if __name__ == "__main__":
    main()
