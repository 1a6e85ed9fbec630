"""Measurement of NOTES.md beside this file: FASTA text staged by xm_batch_stage_fasta against the host reader over the same files - one block of configs[4]'s
shape (10 kb reads wrapped at 70 columns, split at 1000) and of configs[1]'s (150-base reads, one line each), the gather kernel's share at 60, 70 and 80 columns
and on one-line records, the command-line jobs' phases with and without --parse-on-gpu --fasta-on-gpu, and the launches of an unflagged job."""
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
REPS = 6  # the first call of a shape allocates the context's buffers and is reported apart
out = {}
d = tempfile.mkdtemp()


def fasta_file(path, n, length, width, rng):
    """n records of `length` random bases wrapped at `width` columns (0: one line), written without a Python loop per base."""
    width = width or length
    full, rest = divmod(length, width)
    header = 12
    row = header + full * (width + 1) + ((rest + 1) if rest else 0)
    rows = np.empty((n, row), dtype=np.uint8)
    rows[:, :header] = np.frombuffer(b">read000000\n", dtype=np.uint8)
    for k in range(6):
        rows[:, 5 + k] = 48 + (np.arange(n) // 10 ** (5 - k)) % 10
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, length), dtype=np.uint8)]
    body = rows[:, header:header + full * (width + 1)].reshape(n, full, width + 1)
    body[:, :, :width] = bases[:, :full * width].reshape(n, full, width)
    body[:, :, width] = 10
    if rest:
        rows[:, -rest - 1:-1] = bases[:, full * width:]
        rows[:, -1] = 10
    rows.tofile(path)
    return os.path.getsize(path)


def spread(values):
    v = sorted(values)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def stage_and_read(db, path, split, keep=False):
    """REPS times: the cutter, stage_fastq, and the host reader over the same file -> the first repetition, and the spread of the others."""
    rows, reader = [], []
    for rep in range(REPS):
        t0 = time.perf_counter()
        blocks = list(hostio.read_text_blocks(path, batch_size=10_000_000, keep_qualities=keep, split=split, fasta=True))
        t1 = time.perf_counter()
        assert len(blocks) == 1
        db.stage_fastq(blocks[0])
        t2 = time.perf_counter()
        db.unstage()
        rows.append({"queries": len(blocks[0]), "cut_s": t1 - t0, "stage_call_s": t2 - t1, **{k + "_ms": v for k, v in blocks[0].times_ms.items()}})
        blocks[0].close()
    for rep in range(REPS):
        t0 = time.perf_counter()
        nq = 0
        for b in hostio.read_batches(path, None, 10_000_000, split=split, keep_qualities=keep):
            nq += len(b)
            b.close()
        reader.append(time.perf_counter() - t0)
        assert nq == rows[0]["queries"]
    warm = rows[1:]
    return {"queries": rows[0]["queries"], "first": rows[0], "warm": {k: spread([r[k] for r in warm]) for k in rows[0] if k != "queries"}, "host_reader_first_s": reader[0],
            "host_reader_warm_s": spread(reader[1:])}


rng = np.random.default_rng(18)
ref = synth.synthetic_reference(300_000, seed=0x5EC7)
db = api.ReferenceDatabase([("syn", ref)])
# ---- one block of configs[4]'s shape: 20 000 reads of 10 kb at 70 columns (203 MB), split at 1000, 200 000 queries
big = os.path.join(d, "long70.fa")
out["long70_bytes"] = fasta_file(big, 20_000, 10_000, 70, rng)
out["long70"] = stage_and_read(db, big, 1000)
print(json.dumps({"long70": out["long70"]}), flush=True)
# ---- the gather's share by column width: 5 000 reads of 10 kb (51 MB), split at 1000
for width in (60, 70, 80, 0):
    path = os.path.join(d, "w%d.fa" % width)
    size = fasta_file(path, 5_000, 10_000, width, rng)
    out["width_%d" % width] = dict(stage_and_read(db, path, 1000), bytes=size)
    os.remove(path)
print(json.dumps({k: v["warm"]["kernel_ms"] for k, v in out.items() if k.startswith("width_")}), flush=True)
# ---- one block of configs[1]'s shape: 1 000 000 reads of 150 bases, one line each (163 MB), no split
short = os.path.join(d, "short.fa")
out["short_bytes"] = fasta_file(short, 1_000_000, 150, 0, rng)
out["short"] = stage_and_read(db, short, 0)
print(json.dumps({"short": out["short"]}), flush=True)
os.remove(big)
os.remove(short)

# ---- an unflagged job launches what it launched: the align call's kernel launches before and after the context has staged FASTA text
reads = synth.synthetic_single_end(ref, 4096, seed=77)[0]
arrays = api.ReferenceDatabase.batch_arrays([api.Query(r) for r in reads])
before = db.align_arrays(*arrays, api.AlignmentParameters()).kernel_launches
path = os.path.join(d, "tiny.fa")
fasta_file(path, 100, 150, 60, rng)
(block,) = list(hostio.read_text_blocks(path, fasta=True))
db.stage_fastq(block)
db.unstage()
block.close()
out["kernel_launches_of_an_unflagged_align_call"] = {"before": before, "after_staging_fasta": db.align_arrays(*arrays, api.AlignmentParameters()).kernel_launches}
db.close()

# ---- the command-line jobs.  Long: 2 000 reads of 10 kb at 4mild's rates at 70 columns, split at 1000 (20 000 queries); short: 200 000 reads of 150 bases, one line each
starts = (synth.splitmix64(0x12E, 2000) % np.uint64(len(ref) - 12_600)).astype(np.int64)
long_reads = synth.synthetic_long_reads(ref, starts, 10_000, seed=0x12E, sub_rate=0.02, indel_rate=0.002)
with open(os.path.join(d, "job_long.fa"), "wb") as f:
    for i, r in enumerate(long_reads):
        text = DEC[r].tobytes()
        f.write(b">long%d\n" % i + b"".join(text[k:k + 70] + b"\n" for k in range(0, len(text), 70)))
short_reads = synth.synthetic_single_end(ref, 200_000, seed=0x12F)[0]
with open(os.path.join(d, "job_short.fa"), "wb") as f:
    for i, r in enumerate(short_reads):
        f.write(b">short%d\n" % i + DEC[r].tobytes() + b"\n")
with open(os.path.join(d, "ref.fa"), "wb") as f:
    f.write(b">syn\n" + DEC[ref].tobytes() + b"\n")
jobs = {}
for job, queries, fasta_flags in (("long", ["--split-queries-past-size", "1000", "--queries", os.path.join(d, "job_long.fa")], ["--parse-on-gpu", "--split-on-gpu", "--fasta-on-gpu"]),
                                  ("short", ["--queries", os.path.join(d, "job_short.fa")], ["--parse-on-gpu", "--fasta-on-gpu"])):
    for name, flags in (("host", []), ("fasta_on_gpu", fasta_flags)):
        runs = []
        for rep in range(REPS):
            argv = ["--reference", os.path.join(d, "ref.fa")] + queries + ["--out-sam", os.path.join(d, "%s_%s.sam" % (job, name))] + flags
            t0 = time.perf_counter()
            assert cli.run(argv, out=io.StringIO()) == 0
            runs.append(dict(cli.last_timing["phases"], wall=time.perf_counter() - t0))
        jobs["%s_%s" % (job, name)] = {"first": runs[0], "warm": {k: spread([r[k] for r in runs[1:]]) for k in runs[0] if isinstance(runs[0][k], (int, float))}}
    jobs[job + "_sam_identical"] = open(os.path.join(d, job + "_host.sam"), "rb").read() == open(os.path.join(d, job + "_fasta_on_gpu.sam"), "rb").read()
out["jobs"] = jobs
with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fasta_stage.json"), "w") as f:
    json.dump(out, f, indent=1, default=str)
print(json.dumps(out["jobs"], default=str)[:6000])
