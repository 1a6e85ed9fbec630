"""Measurement for profiles/r12/NOTES.md sections 1 and 3: one batch of 1 M configs[1] reads aligned once, then its SAM records formatted on the GPU
(format_sam_last with the host's names, and with the names xm_batch_stage_fastq left in HBM) and by xmio_write_batch to a RAM-backed file at 1, 4, 16 and 32
threads; free HBM before and after the context's first format call.  One JSON object."""
import json, os, sys, tempfile, time, shutil
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import api, hostio, synth, _capi

_capi.check_stamp()
N = 1_000_000
out = {"cpus": len(os.sched_getaffinity(0))}
d = tempfile.mkdtemp(prefix="xm_sam_", dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
try:
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    ref = synth.synthetic_reference(5_000_000, seed=0xEC011)
    reads = synth.synthetic_single_end(ref, N, read_len=150, seed=0x5EED0E2E)[0]
    fq = os.path.join(d, "reads.fq")
    with open(fq, "wb") as f:
        for lo in range(0, N, 100_000):
            f.write(b"".join(b"@r%09d\n" % (lo + i) + dec[r].tobytes() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads[lo:lo + 100_000])))
    db = api.ReferenceDatabase([("ecoli_syn", ref)], mode="mapper", max_query_length=150)
    db.set_sam_contigs(["ecoli_syn"])
    P = api.AlignmentParameters()
    (batch,) = list(hostio.read_batches(fq, batch_size=N))
    db.stage_arrays(*batch.arrays()); db.commit_staged()
    r = db.align_resident(P)
    free0 = api.device_memory(0)[0]
    runs = []
    for rep in range(6):
        t0 = time.perf_counter(); t = db.format_sam_last(batch); wall = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            out["hbm_bytes_taken_by_the_first_call"] = free0 - api.device_memory(0)[0]
            out["text_bytes"], out["records"] = t.bytes, t.records
            with open(os.path.join(d, "gpu.sam"), "wb") as f:
                f.write(t.view())
        runs.append({"h2d_ms": round(t.h2d_ms, 3), "kernel_ms": round(t.kernel_ms, 3), "d2h_ms": round(t.d2h_ms, 3), "wall_ms": round(wall, 2)})
        t.close()
    out["format_sam_last_host_names"] = runs
    host = {}
    for threads in (1, 4, 16, 32):
        host[threads] = []
        for rep in range(3):
            with open(os.path.join(d, "host.sam"), "wb") as f:
                w = hostio.Writer(["ecoli_syn"], f, None, threads=threads)
                t0 = time.perf_counter(); w.write(batch, r); wall = (time.perf_counter() - t0) * 1e3
            host[threads].append({"wall_ms": round(wall, 1), "format_ms": round(w.seconds["format"] * 1e3, 1), "write_ms": round(w.seconds["write"] * 1e3, 1)})
    out["xmio_write_batch_by_threads"] = host
    import filecmp
    out["identical"] = filecmp.cmp(os.path.join(d, "host.sam"), os.path.join(d, "gpu.sam"), shallow=False)
    batch.close()
    (block,) = list(hostio.read_text_blocks(fq, batch_size=N))
    db.stage_fastq(block); db.commit_staged()
    db.align_resident(P)
    runs = []
    for rep in range(6):
        t0 = time.perf_counter(); t = db.format_sam_last(); wall = (time.perf_counter() - t0) * 1e3
        runs.append({"h2d_ms": round(t.h2d_ms, 3), "kernel_ms": round(t.kernel_ms, 3), "d2h_ms": round(t.d2h_ms, 3), "wall_ms": round(wall, 2)})
        t.close()
    out["format_sam_last_names_in_hbm"] = runs
    block.close()
    db.close()
finally:
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
