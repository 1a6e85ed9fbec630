"""Measurement for profiles/r15/NOTES.md section 1: one batch of 1 M configs[1] reads on one context, aligned with the copy of the result streams on and off,
alternating, six times each: xm_result.d2h_ms, the bytes that cross to the host, the pinned pool's high-water mark (read in a child process per setting, so
that one setting's buffers are not the other's), and xm_summary_last's kernel_ms, d2h_ms and wall time with and without the list.  One JSON object."""
import json, os, subprocess, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import api, synth, _capi

_capi.check_stamp()
N = 1_000_000


def setup():
    ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
    reads = synth.synthetic_single_end(ref, N, read_len=150, seed=0x5EED0E2E)[0]
    db = api.ReferenceDatabase([("ecoli_syn", ref)], mode="mapper", max_query_length=150)
    n, L = reads.shape
    mo = np.zeros(2 * n, np.int64); mo[0::2] = np.arange(n) * L
    ml = np.zeros(2 * n, np.int32); ml[0::2] = L
    db.upload_arrays(np.ones(n, np.int32), mo, ml, reads.reshape(-1), np.zeros(n), np.ones(n))
    return db


if len(sys.argv) > 1:  # child: the pinned pool's high-water mark of a process that only ever aligns with this setting (three calls, results dropped in between)
    on = sys.argv[1] == "on"
    db = setup()
    db.set_result_copy(on)
    P = api.AlignmentParameters()
    for _ in range(3):
        r = db.align_resident(P)
        s = db.summary_last(want_unaligned=True)
        s.close()
        del r
    print(json.dumps({"copy": on, "pinned_high_water": _capi.pinned_host_bytes()[1]}))
    sys.exit(0)

out = {"cpus": len(os.sched_getaffinity(0)), "reads": N}
db = setup()
P = api.AlignmentParameters()
db.align_resident(P)  # warm-up
runs = {"on": [], "off": []}
for rep in range(6):
    for on in (True, False):
        db.set_result_copy(on)
        t0 = time.perf_counter(); r = db.align_resident(P); wall = (time.perf_counter() - t0) * 1e3
        crossed = 16 if not on else 4 * r.num_ints + 8 * r.num_dbls + 16 * (len(r) + 1)
        runs["on" if on else "off"].append({"d2h_ms": round(r.d2h_ms, 3), "kernel_ms": round(r.kernel_ms, 2), "align_wall_ms": round(wall, 2), "stream_bytes_to_host": int(crossed)})
        out["num_ints"], out["num_dbls"] = r.num_ints, r.num_dbls
        del r
out["align_resident"] = runs
summ = {"with_list": [], "without_list": []}
for rep in range(6):
    for want in (True, False):
        t0 = time.perf_counter(); s = db.summary_last(want_unaligned=want); wall = (time.perf_counter() - t0) * 1e3
        summ["with_list" if want else "without_list"].append({"kernel_ms": round(s.kernel_ms, 3), "d2h_ms": round(s.d2h_ms, 3), "wall_ms": round(wall, 3),
                                                              "bytes_to_host": 8 * s.num_alignments + 8 * s.num_unaligned + 48})
        out["num_alignments"], out["num_aligned"], out["num_unaligned_listed"] = s.num_alignments, s.num_aligned, max(out.get("num_unaligned_listed", 0), s.num_unaligned)
        s.close()
out["summary_last"] = summ
db.close()
for mode in ("on", "off"):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        print(r.stderr[-2000:], flush=True)
        sys.exit(r.returncode)
    out["pinned_high_water_copy_" + mode] = json.loads(r.stdout.strip().splitlines()[-1])["pinned_high_water"]
print(json.dumps(out))
