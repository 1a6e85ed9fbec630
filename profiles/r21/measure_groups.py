"""Wall times and bytes of --out-mutations' indel events, held by the host (a plain pile-up that keeps the insertion text: the path of the parent commit, which
this tree leaves as it was) and grouped on the device (group_on_gpu=True), over two pile-ups on one GPU; and the fold alone over events that all have one key
and over events that all have their own.

    python measure_groups.py <reference bases> <reads> <repetitions> <tag> [<directory of the result>]      (writes measure_<tag>.json there, or beside this script)
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import oracle_lib
import pileup_workloads as W
from mapper_amd import _capi, api, multi, pileup, synth


def timed(f, reps):
    out, times = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        times.append(time.perf_counter() - t)
    return out, [round(x * 1000, 2) for x in times]


def fold_alone(n, one_key, reps):
    """xm_test_pileup_group over n deletion events in one call - all on one key, or all on their own - -> wall times of the entry (copies up included), groups."""
    L = _capi.lib()
    ev = np.zeros((n, 8), np.int64)
    ev[:, 1] = 5 if one_key else np.arange(n)
    ev[:, 2], ev[:, 3], ev[:, 4], ev[:, 7] = 2, 3, np.arange(n), pileup.UNIT
    off, text = np.zeros(n + 1, np.int64), np.zeros(1, np.uint8)
    call = (_capi.XmTestGroupCall * 1)(_capi.XmTestGroupCall(n, ev.ctypes.data, off.ctypes.data, text.ctypes.data))
    left = [np.zeros((1, 8), np.int64), np.zeros(1, np.int32), np.zeros(2, np.int64), np.zeros(1, np.uint8)]
    times, groups = [], 0
    for _ in range(reps):
        job = _capi.XmTestGroupJob()
        job.fingerprint_bits, job.initial_capacity = 64, 4
        job.num_calls[0], job.calls[0] = 1, C.cast(call, C.POINTER(_capi.XmTestGroupCall))
        job.left_events, job.left_call, job.left_text_off, job.left_text = (a.ctypes.data for a in left)
        calls = C.POINTER(_capi.XmIndelCalls)()
        t = time.perf_counter()
        if L.xm_test_pileup_group(0, C.byref(job), C.byref(calls)):
            raise RuntimeError(L.xm_last_error().decode())
        times.append(round((time.perf_counter() - t) * 1000, 2))
        rows, _, figures = _capi.indel_calls(calls)
        L.xm_indel_calls_free(calls)
        groups = figures["groups"]
        assert job.num_left == 0 and int(rows["support_units"].sum()) == n * pileup.UNIT
    return times, groups


def main():
    ref_len, n_reads, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    tag = sys.argv[4]
    where = sys.argv[5] if len(sys.argv) > 5 else os.path.dirname(os.path.abspath(__file__))
    t0 = time.perf_counter()
    ref = synth.synthetic_reference(ref_len, seed=0xEC011)
    reads = synth.synthetic_single_end(ref[:min(ref_len, 5_000_000)], n_reads, seed=0x5EED0001, indel_prob=0.3)[0]
    half = len(reads) // 2
    batches = [oracle_lib.QueryBatch([W.single(r) for r in part]) for part in (reads[:half], reads[half:])]
    two = multi.MultiGpuDatabase([("r", ref)], [0, 0])
    print("made reference, reads and index in %.1f s" % (time.perf_counter() - t0), flush=True)
    ms = {"held": pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True), "grouped": pileup.MatchDatabase(two.replicas, 0.1, group_on_gpu=True)}
    # pile-ups of their own for the time of add_last: each adds every batch three times, interleaved (the first add of a pile-up allocates)
    clocks = {"held": pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True), "grouped": pileup.MatchDatabase(two.replicas, 0.1, group_on_gpu=True)}
    add_ms = {k: [] for k in ms}
    for rep, b in enumerate(batches):
        two.replicas[rep].align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())
        for m in ms.values():
            m.add_last(None, replica=rep)
        for k in ("held", "grouped") * 3:
            _, t = timed(lambda: clocks[k].add_last(None, replica=rep), 1)
            add_ms[k] += t
    for m in clocks.values():
        m.close()
    events = ms["held"]._events()
    text_bytes = sum(len(t) for t in ms["held"]._texts.values())
    out = {"tag": tag, "reference": ref_len, "reads": n_reads, "replicas": 2, "events": len(events), "insertion_text_bytes": text_bytes, "add_last_ms_three_per_batch": add_ms,
           "host_bytes_held": {"held": 64 * len(events) + 8 * (len(events) + 2) + text_bytes, "grouped": 64 * len(ms["grouped"]._events())},
           "bytes_to_host_per_add": {"held": round((16 * 2 + 64 * len(events) + 8 * (len(events) + 2) + text_bytes) / 2), "grouped": 16 + 32}}
    f = pileup.MutationDetectionParameters.defaultFilter()
    host_held, t_host_held = timed(lambda: ms["held"].mutations(f), reps)
    host_grouped, t_host_grouped = timed(lambda: ms["grouped"].mutations(f), reps)
    host_held2, t_host_held2 = timed(lambda: ms["held"].mutations(f), reps)
    host_grouped2, t_host_grouped2 = timed(lambda: ms["grouped"].mutations(f), reps)
    gpu_held, t_gpu_held = timed(lambda: ms["held"].mutations(f, on_gpu=True), reps + 2)
    gpu_grouped, t_gpu_grouped = timed(lambda: ms["grouped"].mutations(f, on_gpu=True), reps + 2)
    gpu_held2, t_gpu_held2 = timed(lambda: ms["held"].mutations(f, on_gpu=True), reps)
    gpu_grouped2, t_gpu_grouped2 = timed(lambda: ms["grouped"].mutations(f, on_gpu=True), reps)
    figures = dict(ms["grouped"].last_on_gpu)
    groups_held, t_group_held = timed(lambda: ms["held"]._indels(), 3)
    groups_grouped, t_group_grouped = timed(lambda: ms["grouped"]._indels(), 3)
    assert host_held == host_grouped == gpu_held == gpu_grouped == host_held2 == host_grouped2 == gpu_held2 == gpu_grouped2 and groups_held == groups_grouped
    out["default"] = {"rows": len(host_held), "groups": len(groups_held), "host_path_ms": {"held": t_host_held + t_host_held2, "grouped": t_host_grouped + t_host_grouped2},
                      "device_path_ms": {"held": t_gpu_held + t_gpu_held2, "grouped": t_gpu_grouped + t_gpu_grouped2},
                      "grouping_ms": {"held": t_group_held, "grouped_all_groups_down": t_group_grouped},
                      "figures_grouped": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in figures.items()}}
    print(json.dumps(out["default"]), flush=True)
    for name, one_key in (("one_key", True), ("all_distinct", False)):
        t, groups = fold_alone(1_000_000, one_key, reps)
        out["fold_1M_" + name] = {"entry_ms": t, "groups": groups}
        print(json.dumps({name: out["fold_1M_" + name]}), flush=True)
    with open(os.path.join(where, "measure_%s.json" % tag), "w") as fh:
        json.dump(out, fh, indent=1)
    for m in ms.values():
        m.close()
    two.close()


if __name__ == "__main__":
    main()
