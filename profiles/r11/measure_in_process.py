"""Measurement for profiles/r11/NOTES.md: configs[1] FASTQ on disk -> SAM on disk through cli.run with and without --parse-on-gpu (alternating, five each),
the per-batch times of the two staging entries per 1 M reads, and the cutter / the host reader alone on one thread."""
import io, json, os, statistics, sys, tempfile, time, shutil
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import api, cli, hostio, synth, _capi

_capi.check_stamp()
N = 2_000_000
out = {}
d = tempfile.mkdtemp(prefix="xm_fq_", dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
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
    fq = os.path.join(d, "reads.fq")
    rows.tofile(fq)
    out["fastq_bytes"] = os.path.getsize(fq)
    out["bytes_per_record"] = out["fastq_bytes"] / N
    print("files written", flush=True)

    # the cutter and the host reader alone, one thread, file in the page cache
    for name, gen in (("cutter", lambda: hostio.read_text_blocks(fq, batch_size=1_000_000)), ("host_reader", lambda: hostio.read_batches(fq, batch_size=1_000_000))):
        rates = []
        for _ in range(4):
            t0 = time.perf_counter(); n = 0
            for b in gen():
                n += b.num_queries; b.close()
            rates.append(n / (time.perf_counter() - t0) / 1e6)
        out[name + "_Mreads_s"] = [round(r, 3) for r in rates]
    print(json.dumps(out), flush=True)

    # per-batch times per 1 M reads
    db = api.ReferenceDatabase([("ecoli_syn", ref)], mode="mapper", max_query_length=150)
    P = api.AlignmentParameters()
    stage = {"fastq": [], "arrays_h2d_ms": [], "fastq_wall_ms": [], "arrays_wall_ms": []}
    for rep in range(3):
        for b in hostio.read_text_blocks(fq, batch_size=1_000_000):
            t0 = time.perf_counter(); db.stage_fastq(b); stage["fastq_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            stage["fastq"].append({k: round(v, 3) for k, v in b.times_ms.items()})
            db.commit_staged(); b.close()
        for b in hostio.read_batches(fq, batch_size=1_000_000):
            t0 = time.perf_counter(); db.stage_arrays(*b.arrays()); stage["arrays_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 2))
            db.commit_staged(); r = db.align_resident(P); stage["arrays_h2d_ms"].append(round(r.h2d_ms, 3)); b.close()
    db.close()
    out["stage_per_1M_reads"] = stage
    print(json.dumps(stage), flush=True)

    # end to end, alternating
    e2e = {"host": [], "gpu": []}
    sams = {}
    for rep in range(5):
        for mode in ("host", "gpu"):
            log = io.StringIO()
            sam = os.path.join(d, mode + ".sam")
            rc = cli.run(["--reference", os.path.join(d, "ref.fa"), "--queries", fq, "--out-sam", sam] + (["--parse-on-gpu"] if mode == "gpu" else []), out=log)
            t = cli.last_timing
            assert rc == 0 and t["queries"] == N
            e2e[mode].append(round(N / t["stream_seconds"] / 1e6, 4))
            sams[mode] = os.path.getsize(sam)
            print(mode, e2e[mode][-1], t["contexts"], flush=True)
    import filecmp
    out["sam_identical"] = filecmp.cmp(os.path.join(d, "host.sam"), os.path.join(d, "gpu.sam"), shallow=False)
    out["end_to_end_Mreads_s"] = e2e
    out["end_to_end_median"] = {k: statistics.median(v) for k, v in e2e.items()}
finally:
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
