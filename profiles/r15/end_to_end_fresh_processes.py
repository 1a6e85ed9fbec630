"""configs[1] FASTQ on disk (2 M reads, four batches of 500 000) -> SAM on disk through cli.run: no flags, --format-on-gpu, that plus --results-on-gpu, those
plus --parse-on-gpu, and no flags / all flags on three contexts (and, with a checkout of the commit before this one as argv[1], that commit's run without
flags), every run in a fresh process, alternating, argv[2] (default 3) each.  JSON lines, then the summary."""
import filecmp, json, os, shutil, statistics, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import synth
N = 2_000_000
parent = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "-" else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
modes = ["host", "format", "results", "all", "host3", "all3"] + (["parent"] if parent else [])
d = tempfile.mkdtemp(prefix="xm_res_", dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
res = {m: [] for m in modes}
same = {}
try:
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        f.write(b">ecoli_syn\n" + dec[ref].tobytes() + b"\n")
    reads = synth.synthetic_single_end(ref, N, read_len=150, seed=0x5EED0E2E)[0]
    m, L = reads.shape
    head = np.frombuffer(b"@r%09d\n" % 0, dtype=np.uint8)
    rows = np.empty((m, len(head) + L + 3 + L + 1), dtype=np.uint8)
    rows[:, :len(head)] = head
    idx = np.arange(m)
    for k in range(9):
        rows[:, 2 + k] = 48 + (idx // 10 ** (8 - k)) % 10
    rows[:, len(head):len(head) + L] = dec[reads]
    rows[:, len(head) + L:len(head) + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rows[:, len(head) + L + 3:len(head) + 2 * L + 3] = 73
    rows[:, -1] = 10
    rows.tofile(os.path.join(d, "reads.fq"))
    del rows, reads
    for rep in range(reps):
        for mode in modes:
            r = subprocess.run([sys.executable, os.path.join(HERE, "end_to_end_one.py"), d, mode] + ([parent] if mode == "parent" else []), capture_output=True, text=True, timeout=180)
            if r.returncode != 0:
                print(r.stderr[-2000:], flush=True)
                sys.exit(r.returncode)
            line = json.loads(r.stdout.strip().splitlines()[-1])
            res[mode].append(line)
            print(json.dumps(line), flush=True)
    same = {mode: filecmp.cmp(os.path.join(d, "host.sam"), os.path.join(d, mode + ".sam"), shallow=False) for mode in modes[1:]}
finally:
    shutil.rmtree(d, ignore_errors=True)
out = {"runs_Mreads_s": {k: [x["Mreads_s"] for x in v] for k, v in res.items()}, "median_Mreads_s": {k: statistics.median(x["Mreads_s"] for x in v) for k, v in res.items()},
       "median_phases": {k: {p: statistics.median(x["phases"][p] for x in v) for p in v[0]["phases"]} for k, v in res.items()},
       "statistics_identical_to_host": {k: all(x["statistics"] == res["host"][0]["statistics"] for x in v) for k, v in res.items()}, "sam_identical_to_host": same}
print(json.dumps(out))
