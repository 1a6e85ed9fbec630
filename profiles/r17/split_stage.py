"""Measurement of NOTES.md beside this file: one block of configs[4]'s shape staged with split_past_size, the host reader over the same file, and the
command-line job's phases with and without --parse-on-gpu --split-on-gpu."""
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from mapper_amd import api, cli, hostio, synth  # noqa: E402

DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
out = {}
d = tempfile.mkdtemp()

# ---- staging: 10 000 reads of 10 kb (random bases: staging does not look at what they are), 100 000 queries
rng = np.random.default_rng(17)
n = 10_000
rows = np.empty((n, 12 + 10_000 + 3 + 10_000 + 1), dtype=np.uint8)
rows[:, :12] = np.frombuffer(b"@read000000\n", dtype=np.uint8)
for k in range(6):
    rows[:, 5 + k] = 48 + (np.arange(n) // 10 ** (5 - k)) % 10
rows[:, 12:10_012] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 10_000))]
rows[:, 10_012:10_015] = np.frombuffer(b"\n+\n", dtype=np.uint8)
rows[:, 10_015:-1] = 70
rows[:, -1] = 10
big = os.path.join(d, "big.fq")
rows.tofile(big)
out["file_bytes"] = os.path.getsize(big)

ref = synth.synthetic_reference(300_000, seed=0x5EC7)
db = api.ReferenceDatabase([("syn", ref)])
stage = []
for rep in range(4):
    for keep in (False, True):
        t0 = time.perf_counter()
        (block,) = list(hostio.read_text_blocks(big, batch_size=1_000_000, keep_qualities=keep, split=1000))
        t1 = time.perf_counter()
        db.stage_fastq(block)
        t2 = time.perf_counter()
        db.unstage()
        stage.append({"rep": rep, "keep_qualities": keep, "queries": len(block), "cut_s": t1 - t0, "stage_call_s": t2 - t1, **block.times_ms})
        block.close()
out["stage"] = stage
reader = []
for rep in range(3):
    for keep in (False, True):
        t0 = time.perf_counter()
        nq = 0
        for b in hostio.read_batches(big, None, 1_000_000, split=1000, keep_qualities=keep):
            nq += len(b)
            b.close()
        reader.append({"rep": rep, "keep_qualities": keep, "queries": nq, "wall_s": time.perf_counter() - t0})
out["host_reader"] = reader
db.close()
print(json.dumps(out), flush=True)

# ---- the command-line job: 1 000 reads of 10 kb at 4mild's rates (10 000 queries) against the 300 kb reference
starts = (synth.splitmix64(0x10E, 1000) % np.uint64(len(ref) - 12_600)).astype(np.int64)
reads = synth.synthetic_long_reads(ref, starts, 10_000, seed=0x10E, sub_rate=0.02, indel_rate=0.002)
with open(os.path.join(d, "job.fq"), "wb") as f:
    for i, r in enumerate(reads):
        f.write(b"@long%d\n" % i + DEC[r].tobytes() + b"\n+\n" + b"F" * len(r) + b"\n")
with open(os.path.join(d, "ref.fa"), "wb") as f:
    f.write(b">syn\n" + DEC[ref].tobytes() + b"\n")
jobs = {}
for name, flags in (("host", []), ("parse_split_on_gpu", ["--parse-on-gpu", "--split-on-gpu"]),
                    ("host_format_results_on_gpu", ["--format-on-gpu", "--results-on-gpu"]),
                    ("all_on_gpu", ["--parse-on-gpu", "--split-on-gpu", "--format-on-gpu", "--results-on-gpu"])):
    for rep in range(2):
        log = io.StringIO()
        argv = ["--reference", os.path.join(d, "ref.fa"), "--split-queries-past-size", "1000", "--queries", os.path.join(d, "job.fq"), "--out-sam", os.path.join(d, name + ".sam")] + flags
        t0 = time.perf_counter()
        assert cli.run(argv, out=log) == 0
        jobs["%s_%d" % (name, rep)] = {"wall_s": time.perf_counter() - t0, "timing": cli.last_timing}
same = open(os.path.join(d, "host.sam"), "rb").read() == open(os.path.join(d, "all_on_gpu.sam"), "rb").read() == open(os.path.join(d, "parse_split_on_gpu.sam"), "rb").read()
out["jobs"] = jobs
out["sam_identical"] = same
with open(os.path.join(HERE, "split_stage.json"), "w") as f:
    json.dump(out, f, indent=1, default=str)
print(json.dumps(out["jobs"], default=str)[:6000])
print("sam identical:", same)
