"""GPU tier: long reads cut into sections while a batch is staged from FASTQ text (xm_fastq_text.split_past_size, hostio.read_text_blocks(split=...),
`--parse-on-gpu --split-on-gpu`; stages 2a-2c of mapper_amd/csrc/xm_fastq.h over the split form of xm_fastq_rules.h).  The arrays the kernels
build equal the host reader's (hostio.read_batches(split=...), concatenated over its batches) element for element, at the edges of both scans; what is refused
names its record and leaves nothing staged; the sections align as the host reader's do and format with the names the kernels built; the command line writes the
same bytes with and without the two flags, whatever the batch size."""
import ctypes as C
import io
import os
import tempfile

import numpy as np
import pytest

import fastq_cases as fc
import fastq_split_cases as sc
from mapper_amd import _capi, api, cli, hostio, synth

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)


def letters(codes):
    return DEC[codes].tobytes()


def fastq_of(reads, name="r%d", quality=b"I"):
    return b"".join(b"@" + (name % i).encode() + b"\n" + letters(r) + b"\n+\n" + quality * len(r) + b"\n" for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def ref():
    return synth.synthetic_reference(300_000, seed=0x5EC7)


@pytest.fixture(scope="module")
def db(ref):
    d = api.ReferenceDatabase([("syn", ref)])
    d.set_sam_contigs(["syn"])
    yield d
    d.close()


def lines_of(text):
    return text.count(b"\n") + (0 if text.endswith(b"\n") else 1)


def stage_raw(d, text1, split, text2=None, keep=1):
    """xm_batch_stage_fastq on bytes with a split size -> the returned arrays (fastq_cases.batch_dict); ValueError with the library's message."""
    b1 = C.create_string_buffer(text1, len(text1))
    b2 = C.create_string_buffer(text2, len(text2)) if text2 is not None else None
    t = _capi.XmFastqText(C.addressof(b1), len(text1), lines_of(text1) // 4, C.addressof(b2) if b2 is not None else None, len(text2) if b2 is not None else 0,
                          lines_of(text2) // 4 if b2 is not None else 0, 100.0, 50.0, keep, split)
    out = C.POINTER(_capi.XmFastqBatch)()
    if d._L.xm_batch_stage_fastq(d._h, C.byref(t), C.byref(out)):
        assert not out
        raise ValueError(d._L.xm_last_error().decode())
    got = fc.batch_dict(out.contents)
    assert out.contents.store is None and out.contents.h2d_ms >= 0 and out.contents.kernel_ms > 0 and out.contents.d2h_ms >= 0
    d._L.xm_fastq_batch_free(out)
    return got


def check_against_reader(d, tmp_path, what, text, split, keeps=(1, 0)):
    path = fc.write(str(tmp_path / "a.fastq"), text)
    want = None
    for keep in keeps:
        want = sc.reader_arrays(path, split, keep_qualities=bool(keep), batch_size=1000)
        fc.assert_same_arrays(stage_raw(d, text, split, keep=keep), want, (what, split, keep))
    return want


def test_abi_version_is_12():
    assert _capi.lib().xm_abi_version() == 12 == _capi.ABI_VERSION


# ---------------------------------------------------------------- the arrays
@pytest.mark.parametrize("split", sc.SPLITS)
def test_arrays_equal_the_host_readers(db, tmp_path, split):
    for name, text in sorted(sc.texts(split).items()):
        want = check_against_reader(db, tmp_path, name, text, split)
        assert want["num_queries"] == sum(len(cli.split_sections(n, split)) for n in sc.sequence_lengths(text)) and want["mate_length"].max() <= split


def record(name_len, seq_len, k=0):
    seq = bytes(b"ACGT"[(k + i * i) % 4] for i in range(seq_len))
    return b"@" + bytes(b"abcdefghij"[(k + i) % 10] for i in range(name_len)) + b"\n" + seq + b"\n+\n" + bytes(33 + (k + i) % 40 for i in range(seq_len)) + b"\n"


def edge_texts():
    T = _capi.lib().xm_fastq_tile_bytes()
    tail = fc.random_fastq(9, 6)
    return {
        "records_4097": (fc.random_fastq(4097, 9, length=lambda k: 1 + k % 5, name=lambda k: "n" * (k % 3)), 10, 4097),     # one section each: a block of the record scan and one record
        "records_8193": (fc.random_fastq(8193, 10, length=lambda k: 1 + k % 7, name=lambda k: "m" * (k % 2)), 10, 8193),    # two blocks and one record
        "record_over_a_block_of_the_offset_scan": (fc.random_fastq(3, 8) + record(7, 5000) + tail, 2, None),                # 2 500 queries of one record: slot 4 096 lies inside it
        "record_of_30001_bases": (fc.random_fastq(3, 8) + record(4, 30_001) + tail, 1000, 3 + 31 + 9),                      # refused without a split size
        "newline_last_byte_of_a_tile": (record(T - 2, 40) + tail, 7, None),
        "newline_first_byte_of_next_tile": (record(T - 1, 40) + tail, 7, None),
        "sequence_newline_on_both_sides": (record(5, T - 8) + record(4, T - 1 - 7) + tail, 100, None),
        "mixed_counts": (b"".join(record(k % 13, (k * 37) % 211 + 1, k) for k in range(600)), 16, None),                    # 1 .. 14 sections a record, 600 records
    }


@pytest.mark.parametrize("name", ["records_4097", "records_8193", "record_over_a_block_of_the_offset_scan", "record_of_30001_bases", "newline_last_byte_of_a_tile",
                                  "newline_first_byte_of_next_tile", "sequence_newline_on_both_sides", "mixed_counts"])
def test_edges_of_the_scans(db, tmp_path, name):
    text, split, nq = edge_texts()[name]
    T = _capi.lib().xm_fastq_tile_bytes()
    if name == "newline_last_byte_of_a_tile":
        assert text[T - 1:T] == b"\n"
    if name == "newline_first_byte_of_next_tile":
        assert text[T:T + 1] == b"\n"
    want = check_against_reader(db, tmp_path, name, text, split, keeps=(1,))
    assert nq is None or want["num_queries"] == nq
    if name == "record_over_a_block_of_the_offset_scan":
        assert want["num_queries"] > 2500 + 3 and (want["mate_length"][0::2] <= 2).all()


def test_split_size_0_stages_what_the_text_stages_without_the_field(db, tmp_path):
    text = fc.rule_texts()["rules_no_final_newline"] + b"\n" + fc.random_fastq(70, 3)
    path = fc.write(str(tmp_path / "a.fastq"), text)
    for keep in (1, 0):
        got = stage_raw(db, text, 0, keep=keep)
        fc.assert_same_arrays(got, fc.reader_arrays(path, keep_qualities=bool(keep)), ("no split", keep))
        assert got["num_queries"] == lines_of(text) // 4 and (keep == 0 or got["has_qual"][0::2].all())
    with pytest.raises(ValueError, match=r"file 1 record 1: mate length out of range \(1..30000"):  # without a split size the limit is a record's
        stage_raw(db, fc.random_fastq(1, 8) + record(4, 30_001), 0)


# ---------------------------------------------------------------- what the kernels read
def same_streams(got, want):
    return (np.array_equal(got.int_off, want.int_off) and np.array_equal(got.ints, want.ints) and np.array_equal(got.dbl_off, want.dbl_off)
            and np.array_equal(np.asarray(got.dbls).view(np.int64), np.asarray(want.dbls).view(np.int64)))


def long_reads(ref, n, seed, junk=3):
    """n reads of 10 kb at the rates bench.py's 4mild uses (2 % substitutions, 0.2 % indel events per base), and `junk` random ones that align nowhere."""
    starts = (synth.splitmix64(seed, n) % np.uint64(len(ref) - 12_600)).astype(np.int64)
    reads = list(synth.synthetic_long_reads(ref, starts, 10_000, seed=seed, sub_rate=0.02, indel_rate=0.002))
    elsewhere = synth.synthetic_reference(10_000 * junk, seed=seed ^ 0x99)
    reads[n // 2:n // 2] = [elsewhere[10_000 * k:10_000 * (k + 1)] for k in range(junk)]
    return reads


@pytest.fixture(scope="module")
def long_fastq(ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_split_long")
    path = fc.write(str(d / "long.fq"), fastq_of(long_reads(ref, 20, 0x10C), "long%d", quality=b"F"))
    fc.write(str(d / "job.fq"), fastq_of(long_reads(ref, 8, 0x10D, junk=2), "long%d", quality=b"F"))  # the command-line jobs: 100 queries, so that batches of 7 take seconds
    (d / "ref.fa").write_bytes(b">chrA\n" + letters(ref[:180_000]) + b"\n>chrB\n" + letters(ref[180_000:]) + b"\n")
    return d, path


def host_bytes(names, batch, result):
    with tempfile.TemporaryFile("w+b") as f:
        hostio.Writer(names, f, None, threads=2).write(batch, result)
        f.seek(0)
        return f.read()


def test_sections_align_and_format_as_the_host_readers_do(db, long_fastq):
    path = long_fastq[1]
    (block,) = list(hostio.read_text_blocks(path, keep_qualities=True, split=1000))
    assert block.num_queries == 230 and block.longest_line == 1000 and block.split == 1000
    db.stage_fastq(block)
    assert len(block) == 230 and block.times_ms["kernel"] > 0
    db.commit_staged()
    got = db.align_resident(PARAMS)
    text = db.format_sam_last()  # the names the kernels built: every section carries its record's
    (batch,) = list(hostio.read_batches(path, None, 1 << 20, split=1000, keep_qualities=True))
    for a, b in zip(block.arrays(), batch.arrays()):
        assert np.array_equal(a, b)
    want = db.align_arrays(*batch.arrays(), PARAMS)
    assert same_streams(got, want)
    aligned = sum(1 for q in range(230) if got.ints[got.int_off[q] + 1] > 0)
    assert 100 <= aligned <= 200  # most sections of the twenty reads, none of the three that align nowhere
    want_text = host_bytes(["syn"], batch, want)
    assert bytes(text) == want_text and text.records == want_text.count(b"\n") and b"long7\t" in want_text
    assert host_bytes(["syn"], block, got) == want_text  # (the host formatter on the returned names)
    text.close()
    block.close()
    batch.close()


# ---------------------------------------------------------------- refusals
GOOD3 = fc.random_fastq(3, 31)
GOOD2 = fc.random_fastq(2, 32)
BAD = {
    "pairs": (GOOD3, GOOD3, 10, "file 2 record 0: pairs are not cut into sections"),
    "split_over_30000": (GOOD3, None, 30_001, "file 1 record 0: split_past_size out of range (0..30000"),
    "negative_split": (GOOD3, None, -1, "file 1 record 0: split_past_size must be >= 0"),
    "no_bases": (GOOD3 + b"@r\n \t\n+\n\n" + GOOD2, None, 10, "file 1 record 3: mate length out of range"),
    "fasta_record": (GOOD3 + b">f\nACGT\n+\nIIII\n" + GOOD2, None, 10, "file 1 record 3: a FASTA record"),
    "empty_line_between_records": (GOOD3 + b"\n" + GOOD2 + b"@r\nAC\n+\n", None, 10, "file 1 record 3: an empty line"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_name_the_record_and_leave_nothing_staged(db, ref, tmp_path, name):
    text1, text2, split, message = BAD[name]
    reads = synth.synthetic_single_end(ref, 50, seed=25)[0]
    c = db.new_context()
    try:
        c.upload_arrays(*api.ReferenceDatabase.batch_arrays([api.Query(r) for r in reads]))
        before = c.align_resident(PARAMS)
        with pytest.raises(ValueError) as e:
            stage_raw(c, text1, split, text2)
        assert str(e.value).startswith("xm_batch_stage_fastq: " + message), str(e.value)
        with pytest.raises(Exception, match="no staged batch"):
            c.commit_staged()
        after = c.align_resident(PARAMS)  # the resident batch still aligns
        assert same_streams(after, before) and sum(1 for q in range(50) if after.ints[after.int_off[q] + 1] > 0) > 40
        check_against_reader(c, tmp_path, "after " + name, sc.edge_text(10), 10, keeps=(1,))  # and the context then stages a good block
    finally:
        c.close()


# ---------------------------------------------------------------- the command line
def run_job(d, out_dir, args, outputs, flags):
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--reference", str(d / "ref.fa"), "--split-queries-past-size", "1000", "--queries", str(d / "job.fq")] + args
    argv += [x for name in outputs for x in ("--out-" + name, os.path.join(out_dir, name))] + flags
    log = io.StringIO()
    assert cli.run(argv, out=log) == 0
    text = log.getvalue()
    return {name: open(os.path.join(out_dir, name), "rb").read() for name in outputs}, text[text.index("Statistics"):]


SPLIT = ["--parse-on-gpu", "--split-on-gpu"]
JOBS = {
    "batches_of_7": (["--batch-size", "7"], ["sam", "unaligned"], SPLIT),
    "one_batch": (["--batch-size", "100000"], ["sam", "unaligned"], SPLIT),
    "batches_of_7_two_contexts_all_on_gpu": (["--batch-size", "7", "--contexts", "2"], ["sam", "unaligned", "refs-map-count"],
                                             SPLIT + ["--format-on-gpu", "--results-on-gpu", "--count-refs-on-gpu"]),
    "one_batch_all_on_gpu": (["--batch-size", "100000"], ["sam", "unaligned", "refs-map-count"], SPLIT + ["--format-on-gpu", "--results-on-gpu", "--count-refs-on-gpu"]),
    "one_batch_mutations": (["--batch-size", "100000"], ["sam", "mutations"], SPLIT),
}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_command_line_writes_the_same_bytes_with_the_flags(long_fastq, tmp_path, name):
    d = long_fastq[0]
    args, outputs, flags = JOBS[name]
    without = run_job(d, str(tmp_path / "host"), args, outputs, [])
    with_flags = run_job(d, str(tmp_path / "gpu"), args, outputs, flags)
    assert with_flags == without
    assert without[0]["sam"].count(b"\n") >= 40 and "Alignment rate" in without[1]
    if "unaligned" in outputs:
        assert len(without[0]["unaligned"]) >= 20 * 1000 and with_flags[0]["unaligned"].count(b"long") >= 20  # the sections of the two reads that align nowhere, at least
    if "refs-map-count" in outputs:
        assert len(without[0]["refs-map-count"]) > 0


def test_command_line_passes_the_librarys_message_on(long_fastq, tmp_path, capsys):
    d = long_fastq[0]
    bad = fc.write(str(tmp_path / "bad.fq"), GOOD3 + b">f\nACGT\n+\nIIII\n" + GOOD2)
    argv = ["--reference", str(d / "ref.fa"), "--split-queries-past-size", "10", "--queries", bad, "--out-sam", str(tmp_path / "o.sam")]
    rc = cli.main(argv + SPLIT)
    err = capsys.readouterr().err
    assert rc == 1 and "file 1 record 3: a FASTA record" in err and "run without --parse-on-gpu" in err
    assert cli.main(argv) == 0  # (the host reader takes the file)
