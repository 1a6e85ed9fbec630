"""The measurement behind NOTES.md (python profiles/r19/measure_unaligned.py, and again with the argument `repeat`): the command line over bench.py's end_to_end input (5 Mb synthetic reference, 2 M single reads of 150 bases)
with every fifth read made random so that there are unaligned queries, --out-sam and --out-unaligned, with --parse-on-gpu --format-on-gpu --results-on-gpu:
the flags --unaligned-on-gpu --batch-on-gpu off (the parent commit's behaviour) and on, alternating, each job a process of its own."""
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.environ.get("XM_R19_OUT", HERE)  # where measure.json, measure_repeat.json and the trace go
N_READS, READ_LEN, REF_LEN, BATCH = 2_000_000, 150, 5_000_000, 250_000


def make_inputs(d):
    import numpy as np
    from mapper_amd import synth
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    ref = synth.synthetic_reference(REF_LEN, seed=0xEC011)
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        f.write(b">ecoli_syn\n" + dec[ref].tobytes() + b"\n")
    reads = synth.synthetic_single_end(ref, N_READS, read_len=READ_LEN, seed=0x5EED0E2E)[0]
    rng = np.random.default_rng(19)
    reads[4::5] = (1 << rng.integers(0, 4, reads[4::5].shape)).astype(np.uint8)
    m, L = reads.shape
    head = np.frombuffer(b"@r%09d\n" % 0, dtype=np.uint8)
    rows = np.empty((m, len(head) + L + 3 + L + 1), dtype=np.uint8)
    rows[:, :len(head)] = head
    idx = np.arange(m)
    for k in range(9):
        rows[:, 2 + k] = 48 + (idx // 10 ** (8 - k)) % 10
    rows[:, len(head):len(head) + L] = dec[reads]
    rows[:, len(head) + L:len(head) + L + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rows[:, len(head) + L + 3:len(head) + 2 * L + 3] = rng.integers(40, 75, (m, L)).astype(np.uint8)
    rows[:, -1] = 10
    rows.tofile(os.path.join(d, "reads.fq"))


def child(mode, d):
    from mapper_amd import _capi, api, cli
    stage_d2h, texts = [], []
    orig_stage, orig_un = api.ReferenceDatabase.stage_fastq, api.ReferenceDatabase.unaligned_format_last

    def stage(self, block):
        r = orig_stage(self, block)
        stage_d2h.append(block.times_ms["d2h"])
        return r

    def unaligned(self):
        t = orig_un(self)
        texts.append((t.kernel_ms, t.d2h_ms, t.bytes))
        return t
    api.ReferenceDatabase.stage_fastq, api.ReferenceDatabase.unaligned_format_last = stage, unaligned
    argv = ["--reference", os.path.join(d, "ref.fa"), "--queries", os.path.join(d, "reads.fq"), "--batch-size", str(BATCH), "--out-sam", os.path.join(d, mode + ".sam"),
            "--out-unaligned", os.path.join(d, mode + ".un"), "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"]
    if mode == "on":
        argv += ["--unaligned-on-gpu", "--batch-on-gpu"]
    first = None
    if os.environ.get("XM_R19_TWICE"):  # a first job warms the process (runtime, code objects, pinned pool); the second is the one reported
        t0 = time.perf_counter()
        cli.run(argv, out=io.StringIO())
        first = {"wall_seconds": time.perf_counter() - t0, "stream_seconds": cli.last_timing["stream_seconds"], "pinned_high_water": _capi.pinned_host_bytes()[1]}
        del stage_d2h[:], texts[:]
    log = io.StringIO()
    t0 = time.perf_counter()
    rc = cli.run(argv, out=log)
    wall = time.perf_counter() - t0
    digest = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()  # noqa: E731
    stats = log.getvalue()
    print("RESULT " + json.dumps({
        "mode": mode, "rc": rc, "first_job": first, "wall_seconds": wall, "stream_seconds": cli.last_timing["stream_seconds"], "contexts": cli.last_timing["contexts"], "phases": cli.last_timing["phases"],
        "pinned_now": _capi.pinned_host_bytes()[0], "pinned_high_water": _capi.pinned_host_bytes()[1], "stage_d2h_ms": stage_d2h,
        "unaligned_kernel_ms": [t[0] for t in texts], "unaligned_d2h_ms": [t[1] for t in texts], "unaligned_bytes": [t[2] for t in texts],
        "sam": digest(os.path.join(d, mode + ".sam")), "un": digest(os.path.join(d, mode + ".un")), "un_bytes": os.path.getsize(os.path.join(d, mode + ".un")),
        "statistics": stats[stats.index("Statistics"):]}))


def copy_rate(nbytes):
    """A plain device-to-device copy of nbytes on the same GPU (hipMemcpy through torch), best of five after a warm-up -> bytes per second."""
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(65)
    b = torch.empty_like(a)
    best = None
    for k in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if k and (best is None or ms < best):
            best = ms
    print("RESULT " + json.dumps({"copy_bytes": nbytes, "copy_ms": best, "copy_bytes_per_s": nbytes / (best * 1e-3)}))


def run_child(args, limit, prefix=()):
    r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        print("child %s failed with %d\n%s\n%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        sys.exit(1)  # (nothing more is started on the GPU)
    return [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]


def repeat():
    """Four alternations, every process running the job twice: the second, warm job is the one compared."""
    os.makedirs(OUT, exist_ok=True)
    os.environ["XM_R19_TWICE"] = "1"
    with tempfile.TemporaryDirectory(prefix="xm_r19_") as d:
        make_inputs(d)
        runs = []
        for k in range(4):
            for mode in ("off", "on"):
                runs += run_child(["child", mode, d], 240)
                print(mode, "first %.3f s, second %.3f s" % (runs[-1]["first_job"]["stream_seconds"], runs[-1]["stream_seconds"]), "pinned high water after the first %d, after both %d" %
                      (runs[-1]["first_job"]["pinned_high_water"], runs[-1]["pinned_high_water"]), flush=True)
        json.dump({"runs": runs}, open(os.path.join(OUT, "measure_repeat.json"), "w"), indent=1)
        assert len({(r["sam"], r["un"], r["statistics"]) for r in runs}) == 1, "the outputs differ between the runs"


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="xm_r19_") as d:
        make_inputs(d)
        runs = []
        for k in range(3):
            for mode in ("off", "on"):
                runs += run_child(["child", mode, d], 240)
                print(mode, "stream %.3f s" % runs[-1]["stream_seconds"], "pinned high water %d" % runs[-1]["pinned_high_water"], flush=True)
        per_batch = max(runs[1]["unaligned_bytes"])
        copies = run_child(["copy", str(per_batch)], 240)
        trace_dir = os.path.join(OUT, "trace")
        traced = run_child(["child", "on", d], 400, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "--"))
        json.dump({"runs": runs, "copy": copies, "traced_run": traced}, open(os.path.join(OUT, "measure.json"), "w"), indent=1)
        # the kernels' lines of the trace's statistics, beside the rest
        with open(os.path.join(OUT, "kernel_stats.txt"), "w") as out:
            for root, _, files in os.walk(trace_dir):
                for name in files:
                    if name.endswith("kernel_stats.csv"):
                        for line in open(os.path.join(root, name)):
                            if "Name" in line or "xm_unaligned" in line or "xm_fastq_gather" in line or "xm_sam_write" in line or "xm_scan" in line:
                                out.write(line)
        assert len({(r["sam"], r["un"], r["statistics"]) for r in runs}) == 1, "the outputs differ between the runs"
        print("outputs identical over %d runs; unaligned file %d bytes" % (len(runs), runs[0]["un_bytes"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) > 1 and sys.argv[1] == "repeat":
        repeat()
    elif len(sys.argv) > 1 and sys.argv[1] == "copy":
        copy_rate(int(sys.argv[2]))
    else:
        main()
