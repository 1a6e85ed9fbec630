"""bench.py's multi-rank flow without GPUs (round-5 verdict, "multi-GPU readiness without hardware"): `python bench.py --gpus 8 --engine hostsim` starts eight
ranks (fresh child processes, gloo rendezvous on 127.0.0.1), every rank aligns its own shard through the host simulation of the kernel sources, the timed
region is bracketed by barriers, the time is the maximum over the ranks, and rank 0 prints ONE line.  Checked: n_gpus, weak scaling, the ranks' batches differ
pairwise (seed shift 7919 x rank), the value is the whole job's reads over the slowest rank's time.  The line says it is a dry run; it measures nothing."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ranks", [8])
def test_bench_eight_ranks_dry_run_prints_one_rank0_line(ranks):
    reads = 48
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--engine", "hostsim", "--backend", "gloo", "--reads", str(reads), "--ref-len", "60000",
           "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--seed-probes", "0", "--stream-batches", "0", "--single-context-steps", "0", "--wave-steps", "0", "--contexts", "2",
           "--end-to-end-reads", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == ranks and d["scaling"] == "weak" and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert "DRY RUN" in d["data"]
    assert len(d["rank_batch_digests"]) == ranks and len(set(d["rank_batch_digests"])) == ranks   # every rank aligned other reads
    # value = all ranks' reads over the (max-over-ranks) time of the timed steps
    assert abs(d["value"] - ranks * reads * d["steps"] / (d["ms_per_step"] * d["steps"] * 1e-3) / 1e6) <= 1e-3 * max(d["value"], 1e-9) + 1e-4
    assert d["config"]["reads_per_gpu"] == reads and d["config"]["parallelism"] == "reads sharded x%d" % ranks


def test_bench_dump_outputs_dry_run_is_the_same_from_run_to_run(tmp_path):
    """`--dump-outputs DIR`: after the timed steps the result streams of the last step land in DIR as float64 .npy files; the inputs are seeded, so two runs
    with other step counts write the same arrays (rank 0's; two ranks, as the host simulation runs only the multi-rank flow).  --steps is the number of timed steps
    the line reports."""
    import numpy as np
    reads = 40
    got = {}
    for steps in (3, 1):
        d = tmp_path / ("out%d" % steps)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--engine", "hostsim", "--backend", "gloo", "--reads", str(reads), "--ref-len", "60000",
               "--steps", str(steps), "--warmup", "1", "--cpu-sample", "0", "--seed-probes", "0", "--stream-batches", "0", "--single-context-steps", "0", "--wave-steps", "0",
               "--contexts", "1", "--end-to-end-reads", "0", "--dump-outputs", str(d)]
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps
        names = sorted(p.name for p in d.iterdir())
        assert names == ["dbl_off.npy", "dbls.npy", "int_off.npy", "ints.npy", "query_index.npy"]
        arrays = {n[:-4]: np.load(d / n) for n in names}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum((d / n).stat().st_size for n in names) <= 64_000_000
        got[steps] = arrays
    a = got[3]
    assert np.array_equal(a["query_index"], np.arange(reads))   # small enough: every query
    assert a["int_off"][0] == 0 and a["int_off"][-1] == len(a["ints"]) and len(a["int_off"]) == reads + 1 and len(a["ints"]) > reads
    for k in a:
        assert np.array_equal(a[k], got[1][k]), k


def test_bench_dump_outputs_samples_whole_queries_within_the_budget(tmp_path):
    """Streams larger than the budget: whole queries in a fixed seeded order until the budget is used, their ints and dbls exactly as in the result."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    nq = 5000

    class R:
        pass
    r = R()
    ni, nd = rng.integers(2, 30, nq), rng.integers(0, 6, nq)
    r.int_off = np.concatenate([[0], np.cumsum(ni)]).astype(np.int64)
    r.dbl_off = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    r.ints = rng.integers(-2**31, 2**31 - 1, int(r.int_off[-1]), dtype=np.int64).astype(np.int32)
    r.dbls = rng.random(int(r.dbl_off[-1]))
    budget = 100_000
    runs = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        n, total = bench.dump_outputs(r, str(d), budget=budget)
        assert total == nq and 0 < n < nq
        assert sum(p.stat().st_size for p in d.iterdir()) <= budget
        runs.append({p.name: np.load(p) for p in d.iterdir()})
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
    q = runs[0]["query_index.npy"].astype(np.int64)
    assert len(q) == n and np.all(np.diff(q) > 0)
    io, ints, do, dbls = (runs[0][x] for x in ("int_off.npy", "ints.npy", "dbl_off.npy", "dbls.npy"))
    for i, qq in enumerate(q):
        assert np.array_equal(ints[int(io[i]):int(io[i + 1])], r.ints[r.int_off[qq]:r.int_off[qq + 1]])
        assert np.array_equal(dbls[int(do[i]):int(do[i + 1])], r.dbls[r.dbl_off[qq]:r.dbl_off[qq + 1]])


def test_bench_plain_run_measures_the_headline_alone():
    """Without --full a run sets up, warms up, times its steps and prints the line: none of the side measurements or checks runs (their options are left
    at their defaults here, which start every one of them under --full), and the line says so."""
    reads = 40
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--engine", "hostsim", "--reads", str(reads), "--ref-len", "60000", "--steps", "2", "--warmup", "1"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - reads / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * max(d["value"], 1e-9) + 1e-4
    for k in ("single_context", "pcie_inclusive", "streamed", "wave_form", "golden", "cpu_baseline", "bit_identical", "seed_probe"):
        assert d[k] is None, k
    assert "end_to_end" not in d and list(d["counters"]) == ["device"] and d["roofline"]["frac_one_launch_at_a_time"] is None
    assert 0 < d["config"]["aligned_reads"] <= reads and d["roofline"]["algorithmic_bytes_per_step"] > 0   # (from the timed steps' own result)
