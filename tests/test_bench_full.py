"""bench.py on one GPU, plain and with --full, at a small size: the plain run measures the headline alone, --full still runs every side measurement and
check of the line (one context at a time, host buffers in, streamed batches, the wave-per-read form, the CPU oracle with its parity checks, the seed-probe
micro-benchmark on a second index, the command line from FASTQ to SAM) and they pass.  Both align the same batch to the same result."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--reads", "20000", "--ref-len", "1000000", "--steps", "2", "--warmup", "1", "--single-context-steps", "1", "--stream-batches", "2", "--wave-steps", "1",
         "--cpu-sample", "20000", "--cpu-seconds", "0", "--seed-probes", "100000", "--seed-index-mb", "5", "--end-to-end-reads", "20000"]
SIDE = ("single_context", "pcie_inclusive", "streamed", "wave_form", "cpu_baseline", "seed_probe")


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_and_full_run():
    plain = _bench([])
    assert plain["full"] is False and plain["value"] > 0 and plain["roofline"]["frac"] > 0
    assert all(plain[k] is None for k in SIDE) and plain["bit_identical"] is None and "end_to_end" not in plain and list(plain["counters"]) == ["device"]

    full = _bench(["--full"])
    assert full["full"] is True and full["value"] > 0
    assert all(full[k] is not None for k in SIDE), {k: full[k] is not None for k in SIDE}
    assert full["bit_identical"] is True and full["counters"]["equal"] is True and full["wave_form"]["bit_identical_to_default_path"] is True
    assert full["single_context"]["steps"] == 1 and full["streamed"]["batches"] == 2 * full["contexts"]["per_gpu"]
    assert full["cpu_baseline"]["runs"] == 1 and full["seed_probe"]["hbm_resident_index"]["reference_bases"] == 5_000_000
    assert full["end_to_end"]["value"] is not None and full["end_to_end"]["reads"] == 20000

    assert full["counters"]["device"] == plain["counters"]["device"] and full["config"]["aligned_reads"] == plain["config"]["aligned_reads"] > 0.95 * 20000
    assert full["roofline"]["algorithmic_bytes_per_step"] == plain["roofline"]["algorithmic_bytes_per_step"]
