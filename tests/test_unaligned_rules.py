"""The unaligned-query file's text without a GPU: the rules the kernels of xm_unaligned.h apply (mapper_amd/csrc/xm_unaligned_rules.h, plain C++) run by
tests/unaligned_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the runtime), against
the host path - the file hostio.Writer (xmio_write_batch) writes for the same batch and streams; hostio.Writer.write(unaligned_text=) and what it refuses;
xmio_write_summary over a batch that stayed in HBM; the command line's --unaligned-on-gpu and --batch-on-gpu: what they accept and refuse, and the job over a
database that needs no GPU, whose batches have no arrays on the host."""
import ctypes as C
import io
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import sam_cases as sc
import summary_cases as sm
import unaligned_cases as uc
from mapper_amd import api, cli, hostio
from standin_db import StandInDatabase
from test_summary_rules import CannedText, NoStreamsDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
HostWriter = hostio.Writer


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "unaligned_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/unaligned_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("unaligned_rules") / "unaligned_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def formatted(program, tmp_path, batch, streams):
    """The program's text for the case -> (text, mates, unaligned queries), or ("malformed", query)."""
    r = subprocess.run([program, "format", uc.write_case(str(tmp_path / "case.bin"), batch, streams)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    head, _, text = r.stdout.partition(b"\n")
    words = head.split()
    if words[0] == b"malformed":
        return ("malformed", int(words[1]))
    assert words[0] == b"ok" and int(words[1]) == len(text)
    return text, int(words[2]), int(words[3])


def check(program, tmp_path, batch, streams):
    want, _ = uc.expected(batch, streams)
    text, mates, unaligned = formatted(program, tmp_path, batch, streams)
    assert text == want
    listed = sm.recount(streams.arrays() if isinstance(streams, sc.Streams) else streams).unaligned
    assert unaligned == len(listed) and mates == sum(int(batch.mate_count[q]) for q in listed)
    return text, mates, unaligned


# ---------------------------------------------------------------- the rules against the host writer
def test_every_shape_is_written_as_the_host_writes_it(program, tmp_path):
    batch, streams = uc.shapes_case()
    text, mates, unaligned = check(program, tmp_path, batch, streams)
    # (by hand from shapes_case: 18 queries, three of them aligned, one of those a pair; five pairs in all)
    assert unaligned == 15 and mates == 15 + 4
    assert b"@fastq_single\n" in text and b">fasta_single\n" in text and b"aligned" not in text
    assert b"@pair_fq_fa/1\n" in text and b">pair_fq_fa/2\n" in text and b">pair_fa_fq/1\n" in text and b"@pair_fa_fq/2\n" in text
    assert b"\n@\n" in text and b"\n>\n" in text and b"@" + b"n" * 300 + b"\n" in text
    assert b"@one_base\n" in text and b"@sixteen_codes\n?ACMGRSVTWYHKDBN\n+\n" in text and b">sixteen_codes_twice\nNBDKHYWTVSRGMCA??ACMGRSVTWYHKDBN\n" in text
    at = text.index(b"@thirty_thousand\n") + len(b"@thirty_thousand\n")
    assert text[at + 30_000:at + 30_003] == b"\n+\n" and text[at + 60_003:at + 60_004] == b"\n" and len(set(text[at:at + 30_000])) == 16


def test_every_query_unaligned_and_no_query_unaligned(program, tmp_path):
    batch, streams = uc.shapes_case(every=True)
    text, mates, unaligned = check(program, tmp_path, batch, streams)
    assert unaligned == 18 and mates == 23 and b"@pair_aligned/2\n" in text and b">last_aligned\n" in text
    batch, streams = uc.shapes_case(every=False)
    assert check(program, tmp_path, batch, streams) == (b"", 0, 0)


def test_a_batch_without_has_qual_is_all_fasta(program, tmp_path):
    batch, streams = uc.shapes_case()
    plain = uc.without_has_qual(batch)
    assert plain.has_qual is None and not plain._raw.has_qual and not plain._raw.quals
    text, mates, unaligned = check(program, tmp_path, plain, streams)
    assert unaligned == 15 and mates == 19 and b"@" not in text.replace(b">pair", b"") and b"\n+\n" not in text and text.count(b">") >= 19


@pytest.mark.parametrize("unaligned", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_batches(program, tmp_path, seed, unaligned):
    batch, streams = uc.random_case(seed, 400, unaligned=unaligned)
    assert 0 < batch.has_qual.sum() < 2 * len(batch) and batch.mate_count.max() == 2 and batch.mate_count.min() == 1
    text, mates, n = check(program, tmp_path, batch, streams)
    # (at a share of 0 the only unaligned queries are the pairs that fell back and found nothing for either mate: under 1 % of the queries)
    assert (n == 400) if unaligned == 1.0 else (n < 20) if unaligned == 0.0 else (40 < n < 130)
    # qualities per mate, so that pairs of one FASTQ and one FASTA mate occur at random too
    mixed = uc.with_qualities(batch, seed + 50, per_mate=True)
    check(program, tmp_path, mixed, streams)


def test_record_ends_on_both_sides_of_the_tile_multiples(program, tmp_path):
    batch, streams, ends = uc.tile_edge_case(1024)
    text, _, _ = check(program, tmp_path, batch, streams)
    assert len(ends) == 9 and all(text[e - 1:e] == b"\n" for e in ends) and [e % 1024 for e in ends] == [0, 1, 1023] * 3


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # formatRange accepts them when it writes no SAM (tests/test_summary_rules.py)


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_a_malformed_slice_fails_and_names_the_query(program, tmp_path, name):
    """Query 2 of every case is malformed for the SAM formatter and query 4 for everyone; without a SAM file the host rejects query 2 only where the summary's
    walk does (xm_summary_rules.h), and the unaligned-query file follows that walk: the lowest malformed query is named and there is no text."""
    batch, streams, _ = sc.malformed_cases()[name]
    batch = uc.with_qualities(batch, 5)
    lowest = 4 if name in SAM_ONLY else 2
    with pytest.raises(RuntimeError, match="malformed result streams"):
        uc.expected(batch, streams)
    with pytest.raises(sm.Malformed) as e:
        sm.recount(streams.arrays())
    assert e.value.query == lowest
    assert formatted(program, tmp_path, batch, streams) == ("malformed", lowest)


# ---------------------------------------------------------------- hostio.Writer.write(unaligned_text=)
class HbmBatch:
    """What hostio.TextBlock is once a context with set_batch_copy(False) has staged it: the mate counts, offsets and lengths, and no names, codes or qualities."""

    def __init__(self, batch):
        self.num_queries, self.on_host = batch.num_queries, False
        self._keep = batch
        raw = batch._raw
        self._raw = hostio.XmioBatch(raw.num_queries, raw.mate_count, raw.mate_offset, raw.mate_length, None, raw.codes_length, None, None, None, None, None, None)
        self._ptr = C.pointer(self._raw)


def without_list(summary):
    summary.unaligned, summary.num_unaligned = np.zeros(0, np.int64), 0
    return summary


def test_the_writer_writes_the_text_as_it_is_and_counts_what_the_host_path_counts(tmp_path):
    with open(tmp_path / "host.un", "w+b") as a, open(tmp_path / "text.un", "w+b") as b, open(tmp_path / "hbm.un", "w+b") as c:
        host, by_text, hbm = (hostio.Writer(sc.CONTIGS, None, f, threads=2) for f in (a, b, c))
        for seed in (21, 22, 23):
            batch, streams = uc.random_case(seed, 300, unaligned=0.3)
            arrays = streams.arrays()
            host.write(batch, sc.Result(arrays))
            text, _ = uc.expected(batch, arrays)
            by_text.write(batch, None, summary=without_list(sm.recount(arrays)), unaligned_text=text)
            hbm.write(HbmBatch(batch), None, summary=without_list(sm.recount(arrays)), unaligned_text=memoryview(text))
            assert uc.stats_bits(by_text.stats) == uc.stats_bits(host.stats) == uc.stats_bits(hbm.stats)
        for f in (a, b, c):
            f.seek(0)
        want = a.read()
        assert b.read() == want and c.read() == want and want.count(b"\n+\n") > 60
    assert host.stats.num_queries == 900 and host.stats.total_penalty > 100


def test_what_the_writer_refuses(tmp_path):
    batch, streams = uc.random_case(24, 100, unaligned=0.3)
    arrays = streams.arrays()
    text, _ = uc.expected(batch, arrays)
    with open(tmp_path / "refused.un", "w+b") as f, open(tmp_path / "refused.sam", "w+b") as sam:
        w = hostio.Writer(sc.CONTIGS, sam, f, threads=1)
        with pytest.raises(ValueError, match="comes with a summary"):
            w.write(batch, sc.Result(arrays), unaligned_text=text)
        # an unaligned-query file, a batch without arrays on the host, and no text: with and without a summary
        with pytest.raises(ValueError, match="stayed in HBM.*the text must be given"):
            w.write(HbmBatch(batch), None, sam_text=b"", summary=sm.recount(arrays))
        with pytest.raises(ValueError, match="stayed in HBM.*the text must be given"):
            w.write(HbmBatch(batch), sc.Result(arrays))
        f.seek(0); sam.seek(0)
        assert f.read() == b"" and sam.read() == b"" and w.stats.num_queries == 0
    # the host's formatter reads the batch's arrays: streams instead of a summary are refused for such a batch, whatever the files
    with open(tmp_path / "refused.sam", "w+b") as sam:
        with pytest.raises(ValueError, match="stayed in HBM.*give a summary"):
            hostio.Writer(sc.CONTIGS, sam, None, threads=1).write(HbmBatch(batch), sc.Result(arrays))
        sam.seek(0)
        assert sam.read() == b""
    # without an unaligned-query file such a batch needs no text
    w = hostio.Writer(sc.CONTIGS, None, None)
    w.write(HbmBatch(batch), None, summary=sm.recount(arrays))
    assert w.stats.num_queries == 100


def test_write_summary_over_a_batch_without_names_fails_cleanly(tmp_path):
    batch, streams = uc.random_case(25, 100, unaligned=0.3)
    summary = sm.recount(streams.arrays())
    assert summary.num_unaligned > 10
    pen = np.ascontiguousarray(summary.penalties, np.float64)
    un = np.ascontiguousarray(summary.unaligned, np.int64)
    L = hostio.lib()
    for spoil in ("names", "codes"):
        hbm = HbmBatch(batch)
        if spoil == "names":
            hbm._raw.codes = batch._raw.codes
        else:
            hbm._raw.names, hbm._raw.name_off = batch._raw.names, batch._raw.name_off
        with open(tmp_path / "summary.un", "w+b") as f:
            stats = hostio.XmioStats()
            rc = L.xmio_write_summary(hbm._ptr, summary.num_aligned, summary.total_aligned_length, summary.num_indels, len(pen), pen.ctypes.data, len(un), un.ctypes.data, f.fileno(), C.byref(stats))
            assert rc != 0 and "has no names or codes on the host" in L.xmio_last_error().decode()
            f.seek(0)
            assert f.read() == b"" and stats.num_queries == 0
            # without a file, or without a list, the same batch is only counted
            assert L.xmio_write_summary(hbm._ptr, summary.num_aligned, summary.total_aligned_length, summary.num_indels, len(pen), pen.ctypes.data, len(un), un.ctypes.data, -1, C.byref(stats)) == 0
            assert L.xmio_write_summary(hbm._ptr, summary.num_aligned, summary.total_aligned_length, summary.num_indels, len(pen), pen.ctypes.data, 0, None, f.fileno(), C.byref(stats)) == 0
            assert stats.num_queries == 200


# ---------------------------------------------------------------- the command line
def test_cli_flags_and_what_they_need():
    ref, q = ["--reference", "r.fa"], ["--queries", "q.fq"]
    un, sam = ["--out-unaligned", "u.fq"], ["--out-sam", "o.sam", "--format-on-gpu"]
    gpu = ["--parse-on-gpu", "--results-on-gpu"]
    o = cli.parse_args(ref + q + un + gpu + ["--unaligned-on-gpu"])
    assert o["unaligned_on_gpu"] is True and not o.get("batch_on_gpu")
    for ok in (un + ["--unaligned-on-gpu"], un + sam + ["--unaligned-on-gpu"], ["--no-output"], sam, ["--out-mutations", "m.txt"], un + ["--unaligned-on-gpu", "--out-mutations", "m.txt"]):
        assert cli.parse_args(ref + q + ok + gpu + ["--batch-on-gpu"])["batch_on_gpu"] is True, ok
    assert not cli.parse_args(ref + q + un).get("unaligned_on_gpu")
    for flags, message in (
            (["--unaligned-on-gpu", "--no-output"] + gpu, "--unaligned-on-gpu has nothing to do without --out-unaligned"),
            (un + ["--unaligned-on-gpu", "--results-on-gpu"], "--unaligned-on-gpu needs --parse-on-gpu"),
            (un + ["--unaligned-on-gpu", "--parse-on-gpu"], "--unaligned-on-gpu needs --results-on-gpu"),
            (un + ["--unaligned-on-gpu", "--per-object"], "--unaligned-on-gpu and --per-object exclude each other"),
            (["--no-output", "--batch-on-gpu", "--results-on-gpu"], "--batch-on-gpu needs --parse-on-gpu"),
            (["--no-output", "--batch-on-gpu", "--parse-on-gpu"], "--batch-on-gpu needs --results-on-gpu"),
            (un + gpu + ["--batch-on-gpu"], "--batch-on-gpu with --out-unaligned needs --unaligned-on-gpu"),
            (["--no-output", "--batch-on-gpu", "--per-object"], "--batch-on-gpu and --per-object exclude each other")):
        with pytest.raises(cli.UsageError, match=message):
            cli.parse_args(ref + q + flags)


class ResidentDatabase(NoStreamsDatabase):
    """The stand-in as a context that parses text blocks and, with set_batch_copy(False), keeps what it built to itself: a block is parsed here in Python
    (four-line records, names without blanks) and attached with the mate counts, offsets and lengths alone; the SAM text and the unaligned queries' text of
    the last batch come from what the oracle aligned and the real writer (canned, as far as the command line can tell)."""
    batch_copy = True

    def set_batch_copy(self, on):
        self.batch_copy = bool(on)

    def stage(self, block):
        assert isinstance(block, hostio.TextBlock) and not block.paired and not block.fasta
        lines = block.text().split(b"\n")
        n = block.records()
        reads = [(api.encode(lines[4 * k + 1].decode()),) for k in range(n)]
        names = [(lines[4 * k][1:],) for k in range(n)]
        quals = [(lines[4 * k + 3],) for k in range(n)] if block.keep_qualities else None
        full = uc.Batch(reads, names, quals)
        raw = full._raw
        on = self.batch_copy
        staged = api._capi.XmFastqBatch(n, raw.mate_count, raw.mate_offset, raw.mate_length, raw.codes if on else None, raw.codes_length, raw.names if on else None,
                                        raw.name_off if on else None, raw.quals if on else None, raw.qual_off if on else None, raw.has_qual if on else None, None, 0.0, 0.0, 0.0)
        block.attach(C.pointer(staged), lambda ptr: None)
        self.current = block._keep = full  # (the arrays live as long as the block: the writer thread reads them after the next one is staged)
        assert block.on_host is on and (block.codes is None) is (not on)
        count, offset, length, _, inner, deviation = block.arrays()
        return count, offset, length, full.codes, inner, deviation  # (the oracle aligns what the context kept)

    def align_stream(self, batches, parameters, on_aligned=None):
        return super().align_stream((self.stage(b) for b in batches), parameters, on_aligned=on_aligned)

    def format_sam_last(self, batch=None):
        return super().format_sam_last(self.current if batch is None else batch)

    def unaligned_format_last(self):
        with tempfile.TemporaryFile("w+b") as f:
            HostWriter(self.sam_contigs if hasattr(self, "sam_contigs") else ["x"] * 8, None, f, threads=1).write(self.current, sc.Result(self.last))
            f.seek(0)
            return CannedText(f.read(), NoStreamsDatabase.held)

    def summary_last(self, want_unaligned=False):
        self.asked_for_the_list = getattr(self, "asked_for_the_list", 0) + (1 if want_unaligned else 0)
        return super().summary_last(want_unaligned)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from mapper_amd import synth
    d = tmp_path_factory.mktemp("batch_on_gpu")
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    text = lambda codes: dec[codes].tobytes().decode()  # noqa: E731
    rng = np.random.default_rng(8)
    ref = synth.synthetic_reference(20_000, seed=0xEC011)
    elsewhere = synth.synthetic_reference(5_000, seed=99)
    (d / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n" % (text(ref[:12_000]), text(ref[12_000:])))
    reads = np.concatenate([synth.synthetic_single_end(ref[:12_000], 120, seed=5)[0], synth.synthetic_single_end(elsewhere, 20, seed=6)[0],
                            synth.synthetic_single_end(ref[:12_000], 60, seed=7)[0]])
    (d / "se.fq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, text(r).encode(), uc.quality(rng, len(r)).replace(b" ", b"!")) for i, r in enumerate(reads)))
    return ["--reference", str(d / "ref.fa"), "--queries", str(d / "se.fq"), "--batch-size", "64", "--contexts", "1"]


def run_job(argv, database):
    StandInDatabase.opened.clear()
    NoStreamsDatabase.held.clear()
    log = io.StringIO()
    assert cli.run(argv, out=log, open_database=database) == 0
    assert len(StandInDatabase.opened) == 1 and StandInDatabase.opened[0].closed
    return log.getvalue()


def test_the_job_with_both_flags_writes_the_host_paths_files(job, tmp_path):
    outs = {}
    gpu = ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"]
    for mode, flags, database in (("host", [], StandInDatabase), ("copies", gpu, ResidentDatabase), ("text", gpu + ["--unaligned-on-gpu"], ResidentDatabase),
                                  ("both", gpu + ["--unaligned-on-gpu", "--batch-on-gpu"], ResidentDatabase)):
        sam_path, un_path = str(tmp_path / (mode + ".sam")), str(tmp_path / (mode + ".un"))
        log = run_job(job + ["--out-sam", sam_path, "--out-unaligned", un_path] + flags, database)
        outs[mode] = (open(sam_path, "rb").read(), open(un_path, "rb").read(), log)
        db = StandInDatabase.opened[0]
        if mode != "host":
            assert db.batch_copy is (mode != "both")
            # four batches: a text and a summary each, and with --unaligned-on-gpu the second text - and then nobody asks for the list
            assert len(NoStreamsDatabase.held) == (8 if mode == "copies" else 12) and all(h.closed for h in NoStreamsDatabase.held)
            assert db.asked_for_the_list == (4 if mode == "copies" else 0)
    assert outs["copies"] == outs["host"] and outs["text"] == outs["host"] and outs["both"] == outs["host"]
    assert outs["host"][1].count(b"\n+\n") >= 20 and outs["host"][1].startswith(b"@r") and " Alignment rate                : 90% of queries (180/200)\n" in outs["host"][2]
    # the unaligned queries alone, and no output at all, with the batch in HBM
    un_path = str(tmp_path / "alone.un")
    log = run_job(job + ["--out-unaligned", un_path, "--parse-on-gpu", "--results-on-gpu", "--unaligned-on-gpu", "--batch-on-gpu"], ResidentDatabase)
    assert open(un_path, "rb").read() == outs["host"][1] and log == outs["host"][2]
    assert len(NoStreamsDatabase.held) == 8 and all(h.closed for h in NoStreamsDatabase.held)
    log = run_job(job + ["--no-output", "--parse-on-gpu", "--results-on-gpu", "--batch-on-gpu"], ResidentDatabase)
    assert log == outs["host"][2] and StandInDatabase.opened[0].batch_copy is False


def test_a_block_that_stayed_in_hbm_has_no_bases_to_index(job):
    db = object.__new__(ResidentDatabase)  # (staging needs no reference)
    db.set_batch_copy(False)
    block = next(hostio.read_text_blocks(job[3], None, 10, keep_qualities=True))
    try:
        db.stage(block)
        assert len(block) == 10 and block.codes is None and block.on_host is False and block.mate_length.max() > 50
        with pytest.raises(ValueError, match="stayed in HBM"):
            block[0]
        db.set_batch_copy(True)
        again = next(hostio.read_text_blocks(job[3], None, 10, keep_qualities=True))
        db.stage(again)
        assert len(again[0]) == 1 and len(again[0][0]) == again.mate_length[0]
        again.close()
    finally:
        block.close()


# ---------------------------------------------------------------- the input of the GPU tier's real alignments
@pytest.mark.parametrize("pairs", [False, True])
def test_every_fifth_read_of_the_real_workload_is_unaligned_and_no_other(pairs):
    """tests/test_gpu_unaligned.py asserts that between 10 % and 50 % of these queries are unaligned: the oracle says it is exactly the fifth that was made so."""
    import oracle_lib
    reads = uc.real_reads(400, seed=43, pairs=pairs)
    assert all(100 <= len(m) <= 150 for r in reads for m in r)
    oracle = oracle_lib.OracleReference(uc.real_reference(), mode="mapper")
    got = oracle.align(oracle_lib.QueryBatch([(list(r), 100.0, 50.0) if pairs else (list(r), 0.0, 1.0) for r in reads]), oracle_lib.make_params())
    summary = sm.recount((got.ints, got.dbls, got.int_off, got.dbl_off), num_contigs=1)
    assert list(summary.unaligned) == list(range(4, 400, 5))
    if not pairs:  # the sections of a split size of 60 (50 to 75 bases each): those of every fifth read are unaligned, and no other
        sections = [(r[0][a:b], i) for i, r in enumerate(reads) for a, b in cli.split_sections(len(r[0]), 60)]
        got = oracle.align(oracle_lib.QueryBatch([([s], 0.0, 1.0) for s, _ in sections]), oracle_lib.make_params())
        summary = sm.recount((got.ints, got.dbls, got.int_off, got.dbl_off), num_contigs=1)
        assert list(summary.unaligned) == [k for k, (_, i) in enumerate(sections) if i % 5 == 4] and len(sections) > 800
