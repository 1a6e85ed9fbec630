"""Measurement for profiles/r16/NOTES.md: (1) one batch of 1 M configs[1] reads on one context: xm_refs_count_last's kernel_ms, d2h_ms and wall time, six
times, beside xm_summary_last's on the same resident streams; (2) a job of 100 000 such reads with --out-refs-map-count as its only output, with
--count-refs-on-gpu and without it (the per-object path), each in a fresh child process, alternating after one run that is thrown away: wall time of
cli.run and the process's peak resident set (VmHWM: it starts afresh with the child's program, which ru_maxrss does not).  One JSON object.
argv: nothing (everything), or `job DIR flag|objects` (a child of part 2)."""
import io, json, os, subprocess, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import api, cli, synth, _capi

_capi.check_stamp()
N, JOB = 1_000_000, 100_000

if len(sys.argv) > 1:  # child: one job
    d, mode = sys.argv[2], sys.argv[3]
    log = io.StringIO()
    t0 = time.perf_counter()
    rc = cli.run(["--reference", os.path.join(d, "ref.fa"), "--queries", os.path.join(d, "reads.fq"), "--out-refs-map-count", os.path.join(d, mode + ".txt")] +
                 (["--count-refs-on-gpu"] if mode == "flag" else []), out=log)
    wall = time.perf_counter() - t0
    hwm = [int(line.split()[1]) for line in open("/proc/self/status") if line.startswith("VmHWM:")][0]  # kB
    print(json.dumps({"mode": mode, "rc": rc, "wall_s": round(wall, 2), "stream_s": round(cli.last_timing["stream_seconds"], 2), "contexts": cli.last_timing["contexts"],
                      "peak_rss_mb": round(hwm / 1024, 1), "counts": open(os.path.join(d, mode + ".txt")).read()}))
    sys.exit(0)

out = {"cpus": len(os.sched_getaffinity(0)), "reads": N}
ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
reads = synth.synthetic_single_end(ref, N, read_len=150, seed=0x5EED0E2E)[0]
db = api.ReferenceDatabase([("ecoli_syn", ref)], mode="mapper", max_query_length=150)
n, L = reads.shape
mo = np.zeros(2 * n, np.int64); mo[0::2] = np.arange(n) * L
ml = np.zeros(2 * n, np.int32); ml[0::2] = L
db.upload_arrays(np.ones(n, np.int32), mo, ml, reads.reshape(-1), np.zeros(n), np.ones(n))
P = api.AlignmentParameters()
db.set_result_copy(False)
db.align_resident(P)
db.refs_count_last()  # (the first call allocates the stage's buffers)
runs = {"refs_count_last": [], "summary_last": []}
for rep in range(6):
    t0 = time.perf_counter(); c = db.refs_count_last(raw=True); wall = (time.perf_counter() - t0) * 1e3
    runs["refs_count_last"].append({"kernel_ms": round(c.kernel_ms, 3), "d2h_ms": round(c.d2h_ms, 3), "wall_ms": round(wall, 3)})
    out.update(num_aligned=c.num_aligned, num_combinations=c.num_combinations, num_leftover_queries=c.num_leftover_queries, bytes_to_host=48 * c.num_combinations + 64)
    t0 = time.perf_counter(); s = db.summary_last(want_unaligned=False); wall = (time.perf_counter() - t0) * 1e3
    runs["summary_last"].append({"kernel_ms": round(s.kernel_ms, 3), "d2h_ms": round(s.d2h_ms, 3), "wall_ms": round(wall, 3)})
    s.close()
out["one_batch"] = runs
db.close()

with tempfile.TemporaryDirectory() as d:
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        f.write(b">ecoli_syn\n" + dec[ref].tobytes() + b"\n")
    with open(os.path.join(d, "reads.fq"), "wb") as f:
        f.write(b"".join(b"@r%09d\n" % i + dec[r].tobytes() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads[:JOB])))
    jobs = []
    for mode in ("objects", "flag", "objects", "flag", "objects", "flag", "objects"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "job", d, mode], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(r.stderr[-2000:], flush=True)
            sys.exit(r.returncode)
        jobs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out["same_counts"] = len({j.pop("counts") for j in jobs}) == 1
    jobs = jobs[1:]  # (the first run also fills the file cache)
    out["job_100k"] = jobs
print(json.dumps(out))
