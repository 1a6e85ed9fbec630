"""CPU tier: the command line's one job runner (mapper_amd/cli.py: run, stream, the two sources and the two sinks) over a database that needs no GPU
(tests/standin_db.py: the oracle behind align_stream).  The native path (hostio's reader and Writer) and --per-object write the same bytes; the context
rule; --out-refs-map-count; a sink or a reader that fails mid-job ends the job with its exception and leaves nothing open; the empty jobs."""
import io
import threading
import time

import numpy as np
import pytest

from mapper_amd import cli, hostio, synth
from standin_db import StandInDatabase

DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)


def text(codes):
    return DEC[codes].tobytes().decode()


def fastq(path, reads, name, quality="I"):
    path.write_text("".join("@%s\n%s\n+\n%s\n" % (name % i, text(r), quality * len(r)) for i, r in enumerate(reads)))
    return str(path)


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """The reference (two contigs of 12 000 and 8 000 bases) and the three jobs: name -> (arguments, queries, aligned, records in the unaligned file)."""
    d = tmp_path_factory.mktemp("cli_pipeline")
    ref = synth.synthetic_reference(20_000, seed=0xEC011)
    elsewhere = synth.synthetic_reference(5_000, seed=99)   # reads from here align nowhere
    (d / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n" % (text(ref[:12_000]), text(ref[12_000:])))
    single = np.concatenate([synth.synthetic_single_end(ref[:12_000], 300, seed=5)[0], synth.synthetic_single_end(elsewhere, 30, seed=6)[0]])
    m1, m2 = synth.synthetic_paired_end(ref[12_000:], 100, seed=7)[:2]
    j1, j2 = synth.synthetic_paired_end(elsewhere, 10, seed=8)[:2]
    long_reads = synth.synthetic_single_end(ref[:12_000], 4, read_len=2600, seed=9)[0]
    (d / "long.fa").write_text("".join(">L%d\n%s\n" % (i, text(r)) for i, r in enumerate(long_reads)))
    return {"reference": ["--reference", str(d / "ref.fa")],
            "single": (["--queries", fastq(d / "se.fq", single, "r%d")], 330, 300, 30),
            "paired": (["--paired-queries", fastq(d / "p1.fq", np.concatenate([m1, j1]), "p%d/1", "F"), fastq(d / "p2.fq", np.concatenate([m2, j2]), "p%d/2", "F"),
                        "--spacing", "100", "50"], 110, 100, 20),
            "split": (["--split-queries-past-size", "1000", "--queries", str(d / "long.fa")], 12, 12, 0)}


def run(argv):
    """cli.run over the stand-in -> (return code, log, the database it opened)."""
    StandInDatabase.opened.clear()
    log = io.StringIO()
    rc = cli.run(argv, out=log, open_database=StandInDatabase)
    assert len(StandInDatabase.opened) == 1 and StandInDatabase.opened[0].closed
    return rc, log.getvalue(), StandInDatabase.opened[0]


@pytest.mark.parametrize("contexts", [["--contexts", "1"], []], ids=["one-context", "default-contexts"])
@pytest.mark.parametrize("name", ["single", "paired", "split"])
def test_native_path_equals_per_object_byte_for_byte(jobs, tmp_path, name, contexts):
    args, queries, aligned, unaligned = jobs[name]
    outs = {}
    for mode in ("native", "object"):
        sam_path, un_path = str(tmp_path / (mode + ".sam")), str(tmp_path / (mode + ".un"))
        rc, log, db = run(jobs["reference"] + args + ["--batch-size", "64", "--out-sam", sam_path, "--out-unaligned", un_path] + contexts
                          + (["--per-object"] if mode == "object" else []))
        assert rc == 0
        outs[mode] = (open(sam_path).read(), open(un_path).read(), log)
        # the default rule and the device list (the stand-in ignores the devices): 330 reads are five full batches and more, 110 pairs two batches, 12 sections one
        assert db.devices == [0] * (1 if contexts else {"single": 3, "paired": 2, "split": 1}[name]), mode
    assert outs["native"] == outs["object"]
    sam_text, un_text, log = outs["native"]
    assert " Alignment rate                : %d%% of queries (%d/%d)\n" % (aligned * 100 // queries, aligned, queries) in log
    assert " Average penalty               : " in log and " Num indels                    : " in log
    assert len({l.split("\t")[0] for l in sam_text.splitlines() if not l.startswith("@")}) == {"single": 300, "paired": 200, "split": 4}[name]
    assert un_text.count("\n+\n") == unaligned
    if name == "single":  # exactly the reads from elsewhere, as they came in
        assert [l[1:] for l in un_text.splitlines()[::4]] == ["r%d" % i for i in range(300, 330)]


@pytest.mark.parametrize("explicit,batches,single_short,want", [
    (True, 1, True, 1), (True, 2, True, 1), (True, 5, True, 1), (True, 5, False, 1),   # --devices / --gpus: one context on each
    (False, 0, True, 1), (False, 1, True, 1), (False, 1, False, 1),                     # fewer than two batches
    (False, 2, True, 2), (False, 2, False, 2),                                          # two batches
    (False, 3, True, 3), (False, 4, True, 3), (False, 3, False, 2), (False, 9, False, 2)])
def test_default_contexts(explicit, batches, single_short, want):
    assert cli.default_contexts(explicit, batches, single_short) == want


def test_both_sources_feed_the_context_rule(jobs):
    """The object source gives its real batch count and the facts over all queries; the native one cannot count, so a full first batch stands for
    three batches or more and a short one for the only one, with the facts of the first batch.  The device list is made in one place from either."""
    import contextlib

    def devices(args, batch_size, extra=()):
        o = cli.parse_args(jobs["reference"] + args + ["--no-output", "--batch-size", str(batch_size)] + list(extra))
        with contextlib.ExitStack() as job:
            native = cli.context_devices(o, *cli.native_source(o, batch_size, job)[1:3])
        return native, cli.context_devices(o, *cli.object_source(o, batch_size)[1:3])

    single, paired, split = jobs["single"][0], jobs["paired"][0], jobs["split"][0]
    assert devices(single, 64) == ([0] * 3, [0] * 3)         # 330 short single reads in 6 batches
    assert devices(single, 165) == ([0] * 3, [0] * 2)        # in exactly two: the native reader sees a full first batch, the object path counts two
    assert devices(single, 330) == ([0] * 3, [0])            # in exactly one full batch
    assert devices(single, 331) == ([0], [0])                # a short first batch
    assert devices(paired, 30) == ([0] * 2, [0] * 2)         # pairs: two contexts however many batches
    assert devices(split, 4) == ([0] * 2, [0] * 2)           # sections of 866 bases are single but not short
    assert devices(single, 64, ["--gpus", "2"]) == ([0, 1], [0, 1])
    assert devices(single, 64, ["--devices", "3"]) == ([3], [3])
    assert devices(single, 64, ["--devices", "1,2", "--contexts", "2"]) == ([1, 1, 2, 2], [1, 1, 2, 2])
    assert devices(single, 1000, ["--device", "5", "--contexts", "4"]) == ([5] * 4, [5] * 4)


def test_out_refs_map_count(jobs, tmp_path):
    written = []
    for batch_size in (64, 1000):
        path = tmp_path / ("counts%d.txt" % batch_size)
        rc, log, _ = run(jobs["reference"] + jobs["paired"][0] + ["--out-refs-map-count", str(path), "--batch-size", str(batch_size)])
        assert rc == 0 and "(100/110)" in log
        written.append(path.read_text())
    assert written == ["chrB\t100\n"] * 2


@pytest.fixture
def tracked(monkeypatch):
    """Every batch the native reader hands out and every file cli opens for writing, to be looked at after the job."""
    batches, files = [], []
    read_batches = hostio.read_batches

    def reading(*a, **kw):
        for b in read_batches(*a, **kw):
            batches.append(b)
            yield b

    def opening(path, mode="r"):
        f = open(path, mode)
        if "w" in mode:
            files.append(f)
        return f
    monkeypatch.setattr(hostio, "read_batches", reading)
    monkeypatch.setattr(cli, "open", opening, raising=False)
    return batches, files


def test_a_failing_sink_ends_the_job(jobs, tmp_path, monkeypatch, tracked):
    """20 batches of 32 reads into a sink that takes half a second per batch and fails on its second one: the hand-off queue is full by then, and the job must
    still end - with the sink's exception, every batch closed, the outputs and the database closed, no thread left.  (A writer thread that returns at its
    failure leaves the main thread waiting on the full queue for good: before the runner was one, this job did not end.)"""
    batches, files = tracked
    reads = synth.synthetic_single_end(synth.synthetic_reference(20_000, seed=0xEC011)[:12_000], 640, seed=11)[0]
    queries = fastq(tmp_path / "many.fq", reads, "r%d")

    class FailingWriter(hostio.Writer):
        calls = 0

        def write(self, batch, result):
            FailingWriter.calls += 1
            time.sleep(0.5)
            if FailingWriter.calls == 2:
                raise OSError(28, "No space left on device")
            super().write(batch, result)
    monkeypatch.setattr(hostio, "Writer", FailingWriter)
    threads_before = threading.active_count()
    StandInDatabase.opened.clear()
    raised = []

    def job():
        try:
            cli.run(jobs["reference"] + ["--queries", queries, "--out-sam", str(tmp_path / "out.sam"), "--batch-size", "32", "--contexts", "1"],
                    out=io.StringIO(), open_database=StandInDatabase)
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
    t = threading.Thread(target=job, daemon=True)
    t.start()
    t.join(timeout=60)
    assert not t.is_alive(), "cli.run did not return"
    assert len(raised) == 1 and isinstance(raised[0], OSError) and raised[0].errno == 28
    assert FailingWriter.calls == 2                                    # nothing is written after the failure
    assert 4 <= len(batches) <= 20 and all(b._ptr is None for b in batches)   # (two waiting, one with the sink, one in hand at least were read)
    assert len(files) == 1 and files[0].closed and StandInDatabase.opened[0].closed
    assert threading.active_count() <= threads_before


def test_a_failing_reader_ends_the_job(jobs, tmp_path, tracked):
    """A FASTQ file whose 70th record is cut after its header line: the native reader's ValueError comes out of cli.run, from the third batch, and the
    outputs, the database and the batches are closed."""
    batches, files = tracked
    reads = synth.synthetic_single_end(synth.synthetic_reference(20_000, seed=0xEC011)[:12_000], 69, seed=12)[0]
    path = tmp_path / "cut.fq"
    fastq(path, reads, "r%d")
    path.write_text(path.read_text() + "@r69\n")
    StandInDatabase.opened.clear()
    with pytest.raises(ValueError, match="FASTQ record without a sequence line"):
        cli.run(jobs["reference"] + ["--queries", str(path), "--out-sam", str(tmp_path / "out.sam"), "--out-unaligned", str(tmp_path / "un.fq"), "--batch-size", "32"],
                out=io.StringIO(), open_database=StandInDatabase)
    assert len(batches) == 2 and all(b._ptr is None for b in batches)
    assert len(files) == 2 and all(f.closed for f in files) and StandInDatabase.opened[0].closed


def test_empty_jobs(jobs, tmp_path):
    """What the two paths do with no query at all stays what it was: the native reader's path refuses the job, --per-object reports on nothing."""
    (tmp_path / "none.fq").write_text("")
    argv = jobs["reference"] + ["--queries", str(tmp_path / "none.fq"), "--out-sam", str(tmp_path / "out.sam")]
    StandInDatabase.opened.clear()
    with pytest.raises(cli.UsageError, match="no queries found"):
        cli.run(argv, out=io.StringIO(), open_database=StandInDatabase)
    assert StandInDatabase.opened == []
    rc, log, _ = run(argv + ["--per-object"])
    assert rc == 0 and log.endswith("\nStatistics: \n Alignment rate                : 0% of queries (0/0)\n")
    assert [l for l in open(tmp_path / "out.sam").read().splitlines() if not l.startswith("@")] == []


def test_unequal_pair_files_are_a_usage_error_of_the_object_path(jobs, tmp_path):
    reads = synth.synthetic_single_end(synth.synthetic_reference(20_000, seed=0xEC011)[:12_000], 5, seed=13)[0]
    left, right = fastq(tmp_path / "l.fq", reads, "p%d/1"), fastq(tmp_path / "r.fq", reads[:4], "p%d/2")
    with pytest.raises(cli.UsageError, match="different numbers of reads"):
        cli.run(jobs["reference"] + ["--paired-queries", left, right, "--spacing", "100", "50", "--no-output", "--per-object"], out=io.StringIO(), open_database=StandInDatabase)
