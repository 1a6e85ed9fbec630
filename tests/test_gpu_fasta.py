"""GPU tier: a batch staged from FASTA text whose records span any number of lines (xm_batch_stage_fasta, hostio.read_text_blocks(fasta=True),
`--parse-on-gpu --fasta-on-gpu`; the kernels of mapper_amd/csrc/xm_fasta.h over xm_fasta_rules.h).  The arrays the kernels build equal the host
reader's (hostio.read_batches, concatenated over its batches) element for element, on the CPU tier's texts and at the edges of the tiles, of both line scans,
of the offset scan and of the gather's 64-line window; what is refused names file and record and leaves nothing staged; a staged batch aligns as the host
reader's does and formats with the names the kernels built; the command line writes the same bytes with and without the flags."""
import ctypes as C
import io
import os
import tempfile

import numpy as np
import pytest

import fasta_cases as fa
import fastq_cases as fc
from mapper_amd import _capi, api, cli, hostio, synth

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
EX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples")


def letters(codes):
    return DEC[codes].tobytes()


def fasta_of(reads, width, name="r%d"):
    return b"".join(fa.record((name % i).encode(), letters(r), width) for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def ref():
    return synth.synthetic_reference(300_000, seed=0xFA57A)


@pytest.fixture(scope="module")
def db(ref):
    d = api.ReferenceDatabase([("syn", ref)])
    d.set_sam_contigs(["syn"])
    yield d
    d.close()


def stage_raw(d, text1, split=0, text2=None, keep=1, announce=None):
    """xm_batch_stage_fasta on bytes -> the returned arrays (fastq_cases.batch_dict); ValueError with the library's message.  announce: (records1, lines1, records2,
    lines2) in the place of what the texts hold."""
    b1 = C.create_string_buffer(text1, len(text1))
    b2 = C.create_string_buffer(text2, len(text2)) if text2 is not None else None
    counts = announce or (fa.counts(text1) + (fa.counts(text2) if text2 is not None else (0, 0)))
    t = _capi.XmFastaText(C.addressof(b1), len(text1), counts[0], counts[1], C.addressof(b2) if b2 is not None else None, len(text2) if b2 is not None else 0, counts[2], counts[3],
                          100.0, 50.0, keep, split)
    out = C.POINTER(_capi.XmFastqBatch)()
    if d._L.xm_batch_stage_fasta(d._h, C.byref(t), C.byref(out)):
        assert not out
        raise ValueError(d._L.xm_last_error().decode())
    got = fc.batch_dict(out.contents)
    assert out.contents.store is None and out.contents.h2d_ms >= 0 and out.contents.kernel_ms > 0 and out.contents.d2h_ms >= 0
    d._L.xm_fastq_batch_free(out)
    return got


def check_against_reader(d, tmp_path, what, text, split=0, keeps=(1, 0), text2=None):
    path = fc.write(str(tmp_path / "a.fasta"), text)
    path2 = fc.write(str(tmp_path / "b.fasta"), text2) if text2 is not None else None
    want = None
    for keep in keeps:
        want = fa.reader_arrays(path, path2, split=split, keep_qualities=bool(keep))
        fc.assert_same_arrays(stage_raw(d, text, split, text2, keep=keep), want, (what, split, keep))
    return want


def test_the_entry_came_without_a_new_abi_version():
    assert _capi.lib().xm_abi_version() == 12 == _capi.ABI_VERSION and "xm_batch_stage_fasta" in _capi.EXPORTS


# ---------------------------------------------------------------- the arrays
@pytest.mark.parametrize("split", fa.SPLITS)
def test_arrays_equal_the_host_readers(db, tmp_path, split):
    for name, text in sorted(fa.texts().items()):
        want = check_against_reader(db, tmp_path, name, text, split)
        lengths = fa.record_lengths(text)
        assert want["num_queries"] == (sum(len(cli.split_sections(n, split)) for n in lengths) if split else len(lengths)) and want["mate_length"].sum() == sum(lengths)


def test_pairs_equal_the_host_readers(db, tmp_path):
    a, b = fa.pair_texts()
    want = check_against_reader(db, tmp_path, "pairs", a, text2=b)
    assert want["num_queries"] == 6 and set(want["mate_count"]) == {2}
    want = check_against_reader(db, tmp_path, "pairs swapped", b, text2=a)
    assert want["mate_length"][:2].tolist() == [33, 1]


def named(name_len, seq, width, k=0):
    return fa.record(bytes(b"abcdefghij"[(k + i) % 10] for i in range(name_len)), seq, width)


def edge_texts():
    """name -> (text, split, queries or None)."""
    T = _capi.lib().xm_fastq_tile_bytes()
    tail = fa.wrapped(9, [30, 1, 19])
    one = lambda k: 1 + k % 5  # noqa: E731
    return {
        "header_last_byte_of_a_tile": (named(T - 44, fa.bases(40), 60) + tail, 0, 4),       # the next record's '>' is byte T - 1
        "header_first_byte_of_next_tile": (named(T - 43, fa.bases(40), 60) + tail, 0, 4),   # ... and byte T
        "newline_last_byte_of_a_tile": (b">e\n" + fa.bases(T - 4) + b"\n" + fa.wrap(fa.bases(120, 1), 50) + tail, 0, None),      # a body line's newline is byte T - 1
        "newline_first_byte_of_next_tile": (b">e\n" + fa.bases(T - 3) + b"\n" + fa.wrap(fa.bases(120, 1), 50) + tail, 7, None),  # ... and byte T
        "lines_4097": (b"".join(fa.record(b"l%d" % k, fa.bases(16 * 3 - k % 3, k), 3) for k in range(241)), 0, 241),         # 241 records of 17 lines: a block of the line scan and one line
        "lines_8193": (b"".join(fa.record(b"l%d" % k, fa.bases(6 + k % 4, k), 5) for k in range(2731)), 0, 2731),            # 2 731 records of 3 lines: two blocks and one line
        "records_4097": (b"".join(fa.record(b"n" * (k % 3), fa.bases(one(k), k), 80) for k in range(4097)), 0, 4097),
        "records_8193": (b"".join(fa.record(b"m" * (k % 2), fa.bases(one(k), k), 80) for k in range(8193)), 10, 8193),
        "record_of_4100_lines": (tail + fa.record(b"tall", fa.bases(3 * 4099 - 1), 3) + tail, 0, 7),                         # a block of the line scan lies inside a record
        "record_over_a_block_of_the_offset_scan": (tail + fa.record(b"thin", fa.bases(5000), 1) + tail, 2, None),            # 2 500 queries of one record at width 1: slot 4 096 lies inside it
        "mate_of_30000_bases": (tail + fa.record(b"exact", fa.bases(30_000), 60) + tail, 0, 7),                              # 500 lines
        "record_of_30001_bases": (tail + fa.record(b"long", fa.bases(30_001), 70) + tail, 1000, 3 + 31 + 3),                 # refused without a split size
        "sections_at_line_ends": (b"".join(fa.record(b"s%d" % w, fa.bases(40, w), w) for w in (9, 10, 11)) + tail, 10, None),  # a section ends one base behind, on and one in front of a line end
        "sections_over_lines": (fa.wrapped(7, [250, 333, 100, 101]), 100, None),                                             # width 7, split 100: a section spans fifteen lines
        "split_smaller_than_width": (fa.wrapped(80, [250, 333, 80, 81, 16, 17]), 16, None),
        "records_of_65_to_130_lines": (b"".join(fa.record(b"w%d" % n, fa.bases(3 * (n - 1) - n % 3, n), 3) for n in range(65, 131)), 0, 66),  # the gather's 64-line window is refilled
        "records_of_65_to_130_lines_cut": (b"".join(fa.record(b"w%d" % n, fa.bases(3 * (n - 1) - n % 3, n), 3) for n in range(65, 131)), 200, None),
    }


EDGES = ["header_first_byte_of_next_tile", "header_last_byte_of_a_tile", "lines_4097", "lines_8193", "mate_of_30000_bases", "newline_first_byte_of_next_tile", "newline_last_byte_of_a_tile",
         "record_of_30001_bases", "record_of_4100_lines", "record_over_a_block_of_the_offset_scan", "records_4097", "records_8193", "records_of_65_to_130_lines",
         "records_of_65_to_130_lines_cut", "sections_at_line_ends", "sections_over_lines", "split_smaller_than_width"]


@pytest.mark.parametrize("name", EDGES)
def test_edges(db, tmp_path, name):
    texts = edge_texts()
    assert sorted(texts) == EDGES
    text, split, nq = texts[name]
    T = _capi.lib().xm_fastq_tile_bytes()
    want_byte = {"header_last_byte_of_a_tile": (T - 1, b">"), "header_first_byte_of_next_tile": (T, b">"), "newline_last_byte_of_a_tile": (T - 1, b"\n"),
                 "newline_first_byte_of_next_tile": (T, b"\n")}.get(name)
    if want_byte:
        at, byte = want_byte
        assert text[at:at + 1] == byte and (byte == b"\n" or text[at - 1:at] == b"\n")
    tail_lines = fa.counts(fa.wrapped(9, [30, 1, 19]))[1]
    lines = {"lines_4097": 4097, "lines_8193": 8193, "record_of_4100_lines": 4100 + 2 * tail_lines, "mate_of_30000_bases": 501 + 2 * tail_lines}.get(name)
    assert lines is None or fa.counts(text)[1] == lines
    want = check_against_reader(db, tmp_path, name, text, split, keeps=(1,))
    assert nq is None or want["num_queries"] == nq
    if name == "record_over_a_block_of_the_offset_scan":
        assert want["num_queries"] > 2500 + 6 and (want["mate_length"][0::2] <= 2).all()
    if name == "mate_of_30000_bases":
        assert want["mate_length"].max() == 30_000
    if name == "records_of_65_to_130_lines":
        assert [n.count(b"\n") for n in text.split(b">")[1:]] == list(range(65, 131))


def test_30001_bases_are_refused_without_a_split_size(db):
    text = edge_texts()["record_of_30001_bases"][0]
    with pytest.raises(ValueError, match=r"xm_batch_stage_fasta: file 1 record 3: mate length out of range \(1..30000"):
        stage_raw(db, text)
    assert stage_raw(db, text, 1000)["num_queries"] == 37


# ---------------------------------------------------------------- refusals
GOOD = fa.wrapped(60, [70, 5, 130])
GOOD2 = fa.wrapped(7, [33, 2, 90], name=b"q%d_%d")
R, L = fa.counts(GOOD)
BAD = {
    "first_byte": ((b"ACGT\n" + GOOD, None, 0, None), "file 1 record 0: the text does not start with a FASTA header"),
    "first_byte_of_file_2": ((GOOD, b" " + GOOD2, 0, (R, L, 3, fa.counts(GOOD2)[1])), "file 2 record 0: the text does not start with a FASTA header"),
    "header_after_header": ((GOOD + b">a\n>b\nACGT\n" + GOOD, None, 0, None), "file 1 record 3: mate length out of range"),
    "header_then_blank_lines": ((GOOD + b">a\n\n \t\n\r\n" + GOOD, None, 10, None), "file 1 record 3: mate length out of range"),
    "header_last_line": ((GOOD + b">a", None, 0, None), "file 1 record 3: mate length out of range"),
    "empty_record_in_file_2": ((GOOD, GOOD2.replace(b">q7_1\n", b">q7_1\n>x\n").replace(b">q7_2", b"q7_2"), 0, None), "file 2 record 1: mate length out of range"),
    "lowest_file_and_record": ((GOOD.replace(b">w60_2", b">w60_2 x\n>y"), GOOD2.replace(b">q7_1\n", b">q7_1\n>x\n"), 0, None), "file 1 record 2: mate length out of range"),
    "more_records_announced": ((GOOD, None, 0, (R + 1, L, 0, 0)), "file 1 record 3: the text does not hold the FASTA records announced (3 headers, 4 records announced)"),
    "fewer_records_announced": ((GOOD, None, 7, (R - 1, L, 0, 0)), "file 1 record 2: the text does not hold the FASTA records announced (3 headers, 2 records announced)"),
    "more_lines_announced": ((GOOD, None, 0, (R, L + 1, 0, 0)), "file 1 record 3: the text does not hold the lines announced (9 lines, 10 announced)"),
    "fewer_lines_announced": ((GOOD, None, 7, (R, L - 1, 0, 0)), "file 1 record 3: the text does not hold the lines announced (9 lines, 8 announced)"),
    # bad arguments: refused before anything is queued
    "zero_records": ((GOOD, None, 0, (0, L, 0, 0)), "file 1 record 0: a text holds 1 .. 2^30 bytes and at least one record"),
    "pair_with_a_split": ((GOOD, GOOD2, 10, None), "file 2 record 0: pairs are not cut into sections"),
    "negative_split": ((GOOD, None, -1, None), "file 1 record 0: split_past_size must be >= 0"),
    "split_over_30000": ((GOOD, None, 30_001, None), "file 1 record 0: split_past_size out of range (0..30000"),
    "lines_over_the_cap": ((GOOD, None, 0, (R, (1 << 26) + 1, 0, 0)), "file 1 record 0: a text holds at least a line a record, at most 2^26 lines"),
    "pair_of_3_and_4": ((GOOD, GOOD2 + b">z\nAC\n", 0, None), "file 1 record 3: paired texts have different numbers of records (3, 4)"),
}


def same_streams(got, want):
    return (np.array_equal(got.int_off, want.int_off) and np.array_equal(got.ints, want.ints) and np.array_equal(got.dbl_off, want.dbl_off)
            and np.array_equal(np.asarray(got.dbls).view(np.int64), np.asarray(want.dbls).view(np.int64)))


@pytest.fixture(scope="module")
def resident(db, ref):
    """A context with a resident batch that aligns: what a refusal must leave as it is."""
    reads = synth.synthetic_single_end(ref, 50, seed=25)[0]
    c = db.new_context()
    c.upload_arrays(*api.ReferenceDatabase.batch_arrays([api.Query(r) for r in reads]))
    before = c.align_resident(PARAMS)
    assert sum(1 for q in range(50) if before.ints[before.int_off[q] + 1] > 0) > 40
    yield c, before
    c.close()


@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_name_file_and_record_and_leave_nothing_staged(resident, tmp_path, name):
    (text1, text2, split, announce), message = BAD[name]
    c, before = resident
    with pytest.raises(ValueError) as e:
        stage_raw(c, text1, split, text2, announce=announce)
    assert str(e.value).startswith("xm_batch_stage_fasta: " + message), str(e.value)
    with pytest.raises(Exception, match="no staged batch"):
        c.commit_staged()
    assert same_streams(c.align_resident(PARAMS), before)  # the resident batch still aligns
    check_against_reader(c, tmp_path, "after " + name, GOOD2, 10, keeps=(1,))  # and the context then stages a good block
    c._L.xm_batch_unstage(c._h)


def test_a_null_text_is_refused(db):
    out = C.POINTER(_capi.XmFastqBatch)()
    assert db._L.xm_batch_stage_fasta(db._h, None, C.byref(out)) != 0 and "null argument" in db._L.xm_last_error().decode()
    t = _capi.XmFastaText(None, 10, 1, 2, None, 0, 0, 0, 0.0, 1.0, 0, 0)
    assert db._L.xm_batch_stage_fasta(db._h, C.byref(t), C.byref(out)) != 0 and "file 1 record 0" in db._L.xm_last_error().decode() and not out


# ---------------------------------------------------------------- what the kernels read
def host_bytes(names, batch, result):
    with tempfile.TemporaryFile("w+b") as f:
        hostio.Writer(names, f, None, threads=2).write(batch, result)
        f.seek(0)
        return f.read()


def long_reads(ref, n, seed, junk=2):
    starts = (synth.splitmix64(seed, n) % np.uint64(len(ref) - 12_600)).astype(np.int64)
    reads = list(synth.synthetic_long_reads(ref, starts, 10_000, seed=seed, sub_rate=0.02, indel_rate=0.002))
    elsewhere = synth.synthetic_reference(10_000 * junk, seed=seed ^ 0x99)
    reads[n // 2:n // 2] = [elsewhere[10_000 * k:10_000 * (k + 1)] for k in range(junk)]
    return reads


@pytest.fixture(scope="module")
def files(ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_jobs")
    short = list(synth.synthetic_single_end(ref, 300, seed=0xFA1)[0])
    junk = synth.synthetic_reference(150 * 20, seed=0xFA2)
    short[100:100] = [junk[150 * k:150 * (k + 1)] for k in range(20)]  # twenty reads that align nowhere: the unaligned file has something to hold
    fc.write(str(d / "short.fa"), fasta_of(short, 60, "short%d"))
    m1, m2 = (list(m) for m in synth.synthetic_paired_end(ref, 200, seed=0xFA3)[:2])
    junk = synth.synthetic_reference(150 * 40, seed=0xFA5)
    m1[50:50] = [junk[150 * k:150 * (k + 1)] for k in range(20)]  # twenty pairs that align nowhere
    m2[50:50] = [junk[150 * k:150 * (k + 1)] for k in range(20, 40)]
    fc.write(str(d / "p1.fa"), fasta_of(m1, 60, "pair%d/1"))
    fc.write(str(d / "p2.fa"), fasta_of(m2, 71, "pair%d/2"))
    fc.write(str(d / "long.fa"), fasta_of(long_reads(ref, 8, 0xFA4), 70, "long%d"))
    fc.write(str(d / "reads.fq"), fc.random_fastq(5, 3))
    (d / "ref.fa").write_bytes(b">chrA\n" + letters(ref[:180_000]) + b"\n>chrB\n" + letters(ref[180_000:]) + b"\n")
    return d


@pytest.mark.parametrize("which,split,nq", [("short.fa", 0, 320), ("long.fa", 1000, 100)])
def test_a_staged_batch_aligns_and_formats_as_the_host_readers_does(db, files, which, split, nq):
    path = str(files / which)
    (block,) = list(hostio.read_text_blocks(path, keep_qualities=True, split=split, fasta=True))
    assert block.fasta and block.num_queries == nq and block.longest_line == (1000 if split else 150) and block.lines(0) > 2 * block.records(0)
    db.stage_fastq(block)
    assert len(block) == nq and block.times_ms["kernel"] > 0
    db.commit_staged()
    got = db.align_resident(PARAMS)
    text = db.format_sam_last()  # the names the kernels built
    (batch,) = list(hostio.read_batches(path, None, 1 << 20, split=split, keep_qualities=True))
    for a, b in zip(block.arrays(), batch.arrays()):
        assert np.array_equal(a, b)
    want = db.align_arrays(*batch.arrays(), PARAMS)
    assert same_streams(got, want)
    aligned = sum(1 for q in range(nq) if got.ints[got.int_off[q] + 1] > 0)
    assert (nq // 4 if split else nq // 2) <= aligned <= nq - (20 if not split else 10)
    want_text = host_bytes(["syn"], batch, want)
    assert bytes(text) == want_text and text.records == want_text.count(b"\n") and (b"long7\t" if split else b"short7\t") in want_text
    assert host_bytes(["syn"], block, got) == want_text  # (the host formatter on the returned names)
    text.close()
    block.close()
    batch.close()


# ---------------------------------------------------------------- the command line
def run_job(argv, out_dir, outputs, flags):
    os.makedirs(out_dir, exist_ok=True)
    argv = argv + [x for name in outputs for x in ("--out-" + name, os.path.join(out_dir, name))] + flags
    log = io.StringIO()
    assert cli.run(argv, out=log) == 0
    text = log.getvalue()
    return {name: open(os.path.join(out_dir, name), "rb").read() for name in outputs}, text[text.index("Statistics"):]


FASTA = ["--parse-on-gpu", "--fasta-on-gpu"]
ALL = ["--format-on-gpu", "--results-on-gpu", "--count-refs-on-gpu"]
SHORT = lambda d: ["--reference", str(d / "ref.fa"), "--queries", str(d / "short.fa")]  # noqa: E731
PAIRS = lambda d: ["--reference", str(d / "ref.fa"), "--paired-queries", str(d / "p1.fa"), str(d / "p2.fa"), "--spacing", "100", "50"]  # noqa: E731
LONG = lambda d: ["--reference", str(d / "ref.fa"), "--split-queries-past-size", "1000", "--queries", str(d / "long.fa")]  # noqa: E731
JOBS = {
    "example": (lambda d: ["--reference", os.path.join(EX, "reference.fasta"), "--queries", os.path.join(EX, "queries.fasta")], [], ["sam", "unaligned"], FASTA),
    "short_batches_of_1": (SHORT, ["--batch-size", "1"], ["sam", "unaligned"], FASTA),
    "short_batches_of_7_all_on_gpu": (SHORT, ["--batch-size", "7", "--contexts", "2"], ["sam", "unaligned", "refs-map-count"], FASTA + ALL),
    "short_default_batch": (SHORT, [], ["sam", "unaligned"], FASTA),
    "short_default_batch_all_on_gpu": (SHORT, [], ["sam", "unaligned", "refs-map-count"], FASTA + ALL),
    "short_mutations": (SHORT, [], ["sam", "mutations"], FASTA),
    "pairs": (PAIRS, ["--batch-size", "64"], ["sam", "unaligned"], FASTA),
    "pairs_all_on_gpu": (PAIRS, [], ["sam", "unaligned", "refs-map-count"], FASTA + ALL),
    "long_split_batches_of_7": (LONG, ["--batch-size", "7"], ["sam", "unaligned"], FASTA + ["--split-on-gpu"]),
    "long_split_all_on_gpu": (LONG, [], ["sam", "unaligned", "refs-map-count"], FASTA + ["--split-on-gpu"] + ALL),
    "long_split_mutations": (LONG, [], ["sam", "mutations"], FASTA + ["--split-on-gpu"]),
}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_command_line_writes_the_same_bytes_with_the_flags(files, tmp_path, name):
    argv, args, outputs, flags = JOBS[name]
    without = run_job(argv(files) + args, str(tmp_path / "host"), outputs, [])
    with_flags = run_job(argv(files) + args, str(tmp_path / "gpu"), outputs, flags)
    assert with_flags == without
    assert without[0]["sam"].count(b"\n") >= (3 if name == "example" else 40) and "Alignment rate" in without[1]
    if "unaligned" in outputs:
        assert without[0]["unaligned"].startswith(b">") and b"@" not in without[0]["unaligned"]  # FASTA, as the host writes mates without quality
        assert without[0]["unaligned"].count(b">") >= (1 if name == "example" else 20)
    if "refs-map-count" in outputs:
        assert len(without[0]["refs-map-count"]) > 0
    if "mutations" in outputs:
        assert len(without[0]["mutations"]) > 0


def test_command_line_without_the_flag_refuses_a_fasta_file_as_before(files, tmp_path, capsys):
    argv = SHORT(files) + ["--out-sam", str(tmp_path / "o.sam")]
    rc = cli.main(argv + ["--parse-on-gpu"])
    err = capsys.readouterr().err
    assert rc == 1 and "file 1 record 0: a FASTA record" in err and "run without --parse-on-gpu" in err
    mixed = fc.write(str(tmp_path / "mixed.fq"), fc.random_fastq(3, 1) + b">f\nACGT\n+\nIIII\n" + fc.random_fastq(2, 2))  # a '>' record in the middle of an '@' file: the same refusal with the flag
    for flags in (["--parse-on-gpu"], FASTA):
        rc = cli.main(["--reference", str(files / "ref.fa"), "--queries", mixed, "--out-sam", str(tmp_path / "m.sam")] + flags)
        err = capsys.readouterr().err
        assert rc == 1 and "file 1 record 3: a FASTA record" in err and "run without --parse-on-gpu" in err
    rc = cli.main(["--reference", str(files / "ref.fa"), "--paired-queries", str(files / "p1.fa"), str(files / "reads.fq"), "--spacing", "100", "50", "--out-sam", str(tmp_path / "p.sam")] + FASTA)
    err = capsys.readouterr().err
    assert rc == 1 and "paired query files are of different formats" in err and "p1.fa starts with a FASTA record" in err and "run without --parse-on-gpu" in err
    assert cli.main(SHORT(files) + ["--out-sam", str(tmp_path / "f.sam")] + FASTA) == 0


def test_a_job_without_the_flags_launches_what_it_launched(db, ref):
    """The default path has no new launches: the kernel launches an align call reports for a batch staged from arrays do not depend on the FASTA entry having run
    in the context before (its buffers and kernels are reached through xm_batch_stage_fasta only)."""
    reads = synth.synthetic_single_end(ref, 64, seed=77)[0]
    arrays = api.ReferenceDatabase.batch_arrays([api.Query(r) for r in reads])
    c = db.new_context()
    try:
        before = c.align_arrays(*arrays, PARAMS)
        stage_raw(c, GOOD)
        c._L.xm_batch_unstage(c._h)
        after = c.align_arrays(*arrays, PARAMS)
        assert same_streams(after, before) and after.kernel_launches == before.kernel_launches > 0
    finally:
        c.close()
