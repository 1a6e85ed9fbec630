"""The batch summary without a GPU: the rules the kernels of xm_summary.h apply (mapper_amd/csrc/xm_summary_rules.h, plain C++) run by
tests/summary_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the runtime), against
a recount written in Python from the stream layout (summary_cases.recount); xmio_write_summary against xmio_write_batch without a SAM file; the command
line's --results-on-gpu: what it accepts and refuses, and the job over a database that needs no GPU, whose results carry no streams."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import sam_cases as sc
import summary_cases as sm
from mapper_amd import api, cli, hostio
from standin_db import StandInDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
HostWriter = hostio.Writer  # (the stand-in's canned texts come from the real one, whatever a test puts in its place for the job)


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "summary_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/summary_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("summary_rules") / "summary_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + list(args), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def walk(program, tmp_path, arrays):
    """The program's summary of the streams -> a summary_cases.Summary, or ("malformed", query)."""
    lines = run(program, "walk", sm.write_streams(str(tmp_path / "case.bin"), arrays)).decode().split("\n")
    head = lines[0].split()
    if head[0] == "malformed":
        return ("malformed", int(head[1]))
    assert head[0] == "ok"
    nq, aligned, alignments, length, indels = (int(x) for x in head[1:])
    per_query = [int(x) for x in lines[1].split()]
    penalties = [struct.unpack("<d", bytes.fromhex(x)[::-1])[0] for x in lines[3].split()]
    assert len(per_query) == nq and len(penalties) == alignments == sum(per_query)
    return sm.Summary(nq, aligned, per_query, length, indels, [int(x) for x in lines[2].split()], penalties)


def check(program, tmp_path, streams):
    arrays = sm.arrays_of(streams)
    got, want = walk(program, tmp_path, arrays), sm.recount(arrays)
    assert sm.same(got, want) and got.alignments == want.alignments
    return want


def test_every_shape_is_counted_as_the_recount_counts_it(program, tmp_path):
    want = check(program, tmp_path, sc.shapes_case()[1])
    # (by hand from shapes_case: 25 queries; unaligned_1, unaligned_2 and the fallback pair without alignments; the fallback pair with two alignments per mate has four)
    assert want.num_queries == 25 and list(want.unaligned) == [2, 10, 16] and want.num_aligned == 22 and want.num_indels > 10 and max(want.alignments) == 4


@pytest.mark.parametrize("unaligned", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_streams(program, tmp_path, seed, unaligned):
    want = check(program, tmp_path, sc.random_case(seed, 400, unaligned=unaligned)[1])
    assert want.num_queries == 400
    assert (want.num_unaligned == 400) if unaligned == 1.0 else (want.num_aligned > 250 and want.num_alignments > want.num_aligned and want.num_indels > 0)


def test_unaligned_queries_three_alignments_and_one_pair(program, tmp_path):
    want = check(program, tmp_path, sc.all_unaligned_case(70)[1])
    assert want.num_aligned == 0 and want.num_alignments == 0 and list(want.unaligned) == list(range(70))
    want = check(program, tmp_path, sc.three_alignments_case()[1])
    assert want.alignments == [3] and list(want.penalties) == [1.0, 2.0, 3.0] and want.total_aligned_length == 210
    want = check(program, tmp_path, sc.one_pair_case()[1])
    assert want.alignments == [1] and want.num_indels == 2 and want.total_aligned_length == 32 + 27 and list(want.penalties) == [2.5]
    check(program, tmp_path, sm.many_alignments_case(5, 2))


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # what only a SAM record cannot express: formatRange accepts it when it writes no SAM


def host_accepts(batch, arrays):
    """Whether xmio_write_batch without a SAM file takes the streams."""
    with tempfile.TemporaryFile("w+b") as un:
        try:
            hostio.Writer(sc.CONTIGS, None, un, threads=2).write(batch, sc.Result(arrays))
        except RuntimeError as e:
            assert "malformed result streams" in str(e)
            return False
    return True


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_a_malformed_slice_is_reported_with_its_lowest_query(program, tmp_path, name):
    """Query 2 of every case is malformed for the SAM formatter, and query 4 for everyone (nseq 0).  The conditions that xmio_write_batch rejects without a
    SAM file are reported for query 2; the SAM-only ones are accepted: there the first four queries are counted, and the whole case is malformed at query 4."""
    batch, streams, query = sc.malformed_cases()[name]
    arrays = streams.arrays()
    assert query == 2 and not host_accepts(batch, arrays)
    four = sm.first_queries(arrays, 4)
    four_batch = sc.Batch([(sc.read_of(np.random.default_rng(1), 20),) * int(batch.mate_count[q]) for q in range(4)], [(b"m",) * int(batch.mate_count[q]) for q in range(4)])
    if name in SAM_ONLY:
        assert host_accepts(four_batch, four)
        assert walk(program, tmp_path, arrays) == ("malformed", 4)
        want = check(program, tmp_path, four)
        assert want.num_queries == 4 and want.alignments[2] >= 1
    else:
        assert not host_accepts(four_batch, four)
        assert walk(program, tmp_path, arrays) == ("malformed", 2) and walk(program, tmp_path, four) == ("malformed", 2)
        with pytest.raises(sm.Malformed) as e:
            sm.recount(arrays)
        assert e.value.query == 2


def test_a_slice_cut_short_anywhere_is_malformed_and_nothing_behind_it_is_read(program, tmp_path):
    streams = sc.one_pair_case()[1]
    ints, dbls = len(streams.ints), len(streams.dbls)
    assert ints == 34 and dbls == 8
    out = run(program, "cut", sm.write_streams(str(tmp_path / "pair.bin"), streams.arrays()))  # (every cut in a heap block of its own size: the sanitizer build sees a read behind it)
    assert out.split() == [b"cut", b"ok", b"%d" % ints, b"%d" % dbls], out


# ---------------------------------------------------------------- xmio_write_summary against xmio_write_batch(sam_fd = -1)

class QualBatch(sc.Batch):
    """A sam_cases.Batch some of whose queries came as FASTQ: they carry qualities, and the unaligned-query file shows them."""

    def __init__(self, reads, names, seed):
        super().__init__(reads, names)
        rng = np.random.default_rng(seed)
        n = self.num_queries
        self.has_qual = np.zeros(2 * n, np.uint8)
        self.qual_off = np.zeros(2 * n + 1, np.int64)
        text = []
        for q in range(n):
            fq = rng.random() < 0.5
            for m in range(2):
                k = int(self.mate_length[2 * q + m]) if fq and m < len(reads[q]) else 0
                self.has_qual[2 * q + m] = 1 if fq and m < len(reads[q]) else 0
                text.append(bytes(rng.integers(33, 74, k).astype(np.uint8)))
                self.qual_off[2 * q + m + 1] = self.qual_off[2 * q + m] + k
        self._quals = C.create_string_buffer(b"".join(text), max(int(self.qual_off[-1]), 1))
        self._raw.quals = C.addressof(self._quals)
        self._raw.qual_off = self.qual_off.ctypes.data_as(C.POINTER(C.c_int64))
        self._raw.has_qual = self.has_qual.ctypes.data_as(C.POINTER(C.c_uint8))


def qual_case(seed):
    batch, streams = sc.random_case(seed, 300, unaligned=0.3)
    reads = [tuple(batch.codes[batch.mate_offset[2 * q + m]:batch.mate_offset[2 * q + m] + batch.mate_length[2 * q + m]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    names = [tuple(batch.names[batch.name_off[2 * q + m]:batch.name_off[2 * q + m + 1]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    return QualBatch(reads, names, seed), streams.arrays()


def stats_bits(st):
    return (st.num_queries, st.num_aligned, st.total_aligned_length, st.num_indels, struct.pack("<d", st.total_penalty))


def test_write_summary_equals_write_batch_without_a_sam_file(tmp_path):
    """Three batches one after the other, one running xmio_stats each way: the same unaligned-query file, the same five statistics bit for bit."""
    with open(tmp_path / "streams.un", "w+b") as a, open(tmp_path / "summary.un", "w+b") as b:
        by_streams, by_summary = hostio.Writer(sc.CONTIGS, None, a, threads=2), hostio.Writer(sc.CONTIGS, None, b, threads=2)
        for seed in (21, 22, 23):
            batch, arrays = qual_case(seed)
            assert 0 < batch.has_qual.sum() < 2 * len(batch) and batch.mate_count.max() == 2 and batch.mate_count.min() == 1
            by_streams.write(batch, sc.Result(arrays))
            by_summary.write(batch, None, summary=sm.recount(arrays))
            assert stats_bits(by_summary.stats) == stats_bits(by_streams.stats)
        a.seek(0); b.seek(0)
        text = a.read()
        assert text == b.read() and text.count(b"\n@") > 20 and text.count(b"\n>") > 20 and text.count(b"\n+\n") > 20
    assert by_streams.stats.num_queries == 900 and by_streams.stats.total_penalty > 100 and by_streams.stats.total_penalty != int(by_streams.stats.total_penalty)


def test_write_summary_refuses_a_list_that_is_not_ascending_inside_the_batch(tmp_path):
    batch, arrays = qual_case(24)
    good = sm.recount(arrays)
    assert good.num_unaligned > 10
    for name, spoil in (("descending", lambda u: u[::-1].copy()), ("repeated", lambda u: np.concatenate([u[:1], u[:-1]])), ("behind the batch", lambda u: np.concatenate([u[:-1], [len(batch)]])),
                        ("negative", lambda u: np.concatenate([[-1], u[1:]]))):
        with open(tmp_path / "refused.un", "w+b") as f:
            w = hostio.Writer(sc.CONTIGS, None, f, threads=1)
            bad = sm.recount(arrays)
            bad.unaligned = spoil(good.unaligned).astype(np.int64)
            with pytest.raises(RuntimeError, match="not strictly ascending inside the batch"):
                w.write(batch, None, summary=bad)
            f.seek(0)
            assert f.read() == b"" and w.stats.num_queries == 0, name
    short = sm.recount(arrays)
    short.num_queries -= 1
    with pytest.raises(ValueError, match="summary of 299 queries for a batch of 300"):
        hostio.Writer(sc.CONTIGS, None, None).write(batch, None, summary=short)


# ---------------------------------------------------------------- the command line

def test_cli_flag_and_what_it_excludes():
    ref, q = ["--reference", "r.fa"], ["--queries", "q.fq"]
    sam = ["--out-sam", "o.sam"]
    for ok in (sam + ["--format-on-gpu"], sam + ["--format-on-gpu", "--out-unaligned", "u.fq"], sam + ["--format-on-gpu", "--parse-on-gpu"],
               sam + ["--format-on-gpu", "--parse-on-gpu", "--out-unaligned", "u.fq"], ["--out-unaligned", "u.fq"], ["--no-output"], ["--out-mutations", "m.txt"],
               ["--out-mutations", "m.txt", "--out-unaligned", "u.fq"]):
        assert cli.parse_args(ref + q + ok + ["--results-on-gpu"])["results_on_gpu"] is True, ok
        assert cli.parse_args(ref + ["--results-on-gpu"] + q + ok)["results_on_gpu"] is True, ok
    assert not cli.parse_args(ref + q + sam).get("results_on_gpu")
    with pytest.raises(cli.UsageError, match="--results-on-gpu and --per-object exclude each other"):
        cli.parse_args(ref + q + ["--no-output", "--results-on-gpu", "--per-object"])
    with pytest.raises(cli.UsageError, match="--results-on-gpu and --out-refs-map-count exclude each other"):
        cli.parse_args(ref + q + ["--out-refs-map-count", "c.txt", "--results-on-gpu"])
    with pytest.raises(cli.UsageError, match="--results-on-gpu with --out-sam needs --format-on-gpu"):
        cli.parse_args(ref + q + sam + ["--results-on-gpu"])
    with pytest.raises(cli.UsageError, match="--format-on-gpu and --out-mutations exclude each other"):  # (the existing rule: --out-sam beside --out-mutations stays refused)
        cli.parse_args(ref + q + sam + ["--format-on-gpu", "--results-on-gpu", "--out-mutations", "m.txt"])


class CannedText:
    def __init__(self, data, held):
        self.data, self.closed = data, False
        held.append(self)

    def view(self):
        assert not self.closed
        return memoryview(self.data)

    def close(self):
        self.closed = True


class NoStreamsDatabase(StandInDatabase):
    """The stand-in as a context with set_result_copy(False): its results carry no streams; the text and the summary of the last batch come from what the
    oracle aligned (hostio.Writer's bytes and summary_cases.recount: canned, as far as the command line can tell)."""
    held = []  # every text and summary handed out

    def set_sam_contigs(self, names):
        self.sam_contigs = list(names)

    def set_result_copy(self, on):
        self.result_copy = bool(on)

    def align_stream(self, batches, parameters, on_aligned=None):
        def kept(k):
            if on_aligned is not None:
                on_aligned(k)
        for r in super().align_stream(batches, parameters, on_aligned=None):
            self.last = (r.ints, r.dbls, r.int_off, r.dbl_off)
            kept(getattr(self, "count", 0))
            self.count = getattr(self, "count", 0) + 1
            assert self.result_copy is False
            yield api.BatchResult(dict(ints=None, dbls=None, int_off=None, dbl_off=None, extra=[0] * 8, num_queries=len(r.int_off) - 1))

    def format_sam_last(self, batch=None):
        with tempfile.TemporaryFile("w+b") as f:
            HostWriter(self.sam_contigs, f, None, threads=1).write(batch, sc.Result(self.last))
            f.seek(0)
            return CannedText(f.read(), NoStreamsDatabase.held)

    def summary_last(self, want_unaligned=False):
        s = sm.recount(self.last, num_contigs=1 << 30)
        if not want_unaligned:
            s.unaligned, s.num_unaligned = np.zeros(0, np.int64), 0
        s.closed = False
        s.close = lambda: setattr(s, "closed", True)
        NoStreamsDatabase.held.append(s)
        return s


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from mapper_amd import synth
    d = tmp_path_factory.mktemp("results_on_gpu")
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    text = lambda codes: dec[codes].tobytes().decode()  # noqa: E731
    ref = synth.synthetic_reference(20_000, seed=0xEC011)
    elsewhere = synth.synthetic_reference(5_000, seed=99)
    (d / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n" % (text(ref[:12_000]), text(ref[12_000:])))
    reads = np.concatenate([synth.synthetic_single_end(ref[:12_000], 120, seed=5)[0], synth.synthetic_single_end(elsewhere, 20, seed=6)[0],
                            synth.synthetic_single_end(ref[:12_000], 60, seed=7)[0]])
    (d / "se.fq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, text(r), "I" * len(r)) for i, r in enumerate(reads)))
    return ["--reference", str(d / "ref.fa"), "--queries", str(d / "se.fq"), "--batch-size", "64", "--contexts", "1"]


def run_job(argv, database):
    StandInDatabase.opened.clear()
    NoStreamsDatabase.held.clear()
    log = io.StringIO()
    assert cli.run(argv, out=log, open_database=database) == 0
    assert len(StandInDatabase.opened) == 1 and StandInDatabase.opened[0].closed
    return log.getvalue()


def test_the_job_without_streams_writes_what_the_job_with_streams_writes(job, tmp_path):
    outs = {}
    for mode, flags, database in (("host", [], StandInDatabase), ("gpu", ["--format-on-gpu", "--results-on-gpu"], NoStreamsDatabase)):
        sam_path, un_path = str(tmp_path / (mode + ".sam")), str(tmp_path / (mode + ".un"))
        log = run_job(job + ["--out-sam", sam_path, "--out-unaligned", un_path] + flags, database)
        outs[mode] = (open(sam_path, "rb").read(), open(un_path, "rb").read(), log)
    assert outs["gpu"] == outs["host"]
    assert outs["host"][1].count(b"\n+\n") == 20 and " Alignment rate                : 90% of queries (180/200)\n" in outs["host"][2] and " Average penalty " in outs["host"][2]
    assert len(NoStreamsDatabase.held) == 8 and all(h.closed for h in NoStreamsDatabase.held)   # four batches: a text and a summary each
    assert set(cli.last_timing["phases"]) == {"read", "stage", "align", "format", "write"}
    # the unaligned queries alone, and no output at all: a summary and no text
    un_path = str(tmp_path / "alone.un")
    log = run_job(job + ["--out-unaligned", un_path, "--results-on-gpu"], NoStreamsDatabase)
    assert open(un_path, "rb").read() == outs["host"][1] and log == outs["host"][2]
    assert len(NoStreamsDatabase.held) == 4 and all(h.closed and h.num_unaligned + h.num_aligned == h.num_queries for h in NoStreamsDatabase.held)
    log = run_job(job + ["--no-output", "--results-on-gpu"], NoStreamsDatabase)
    assert log == outs["host"][2]
    assert len(NoStreamsDatabase.held) == 4 and all(h.closed and h.num_unaligned == 0 for h in NoStreamsDatabase.held)


def test_a_writer_that_fails_on_its_second_batch_ends_the_job_and_everything_is_closed(job, tmp_path, monkeypatch):
    class FailingWriter(hostio.Writer):
        calls = 0

        def write(self, batch, result, **kw):
            FailingWriter.calls += 1
            assert kw["sam_text"] is not None and kw["summary"] is not None
            if FailingWriter.calls == 2:
                raise OSError(28, "No space left on device")
            super().write(batch, result, **kw)
    monkeypatch.setattr(hostio, "Writer", FailingWriter)
    StandInDatabase.opened.clear()
    NoStreamsDatabase.held.clear()
    raised = []

    def body():
        try:
            cli.run(job + ["--out-sam", str(tmp_path / "out.sam"), "--out-unaligned", str(tmp_path / "out.un"), "--format-on-gpu", "--results-on-gpu"], out=io.StringIO(),
                    open_database=NoStreamsDatabase)
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(timeout=60)
    assert not t.is_alive(), "cli.run did not return"
    assert len(raised) == 1 and isinstance(raised[0], OSError) and raised[0].errno == 28
    assert FailingWriter.calls == 2
    assert 4 <= len(NoStreamsDatabase.held) <= 8 and all(h.closed for h in NoStreamsDatabase.held)
    assert StandInDatabase.opened[0].closed
