"""GPU tier: a batch staged from FASTQ text (xm_batch_stage_fastq, api.ReferenceDatabase.stage_fastq, `--parse-on-gpu`; the kernels of
mapper_amd/csrc/xm_fastq.h over the rules of xm_fastq_rules.h).  The arrays the kernels build equal the host reader's element for element, at every edge of the
line-end scan; what the align kernels then read gives the result streams of the host reader's arrays bit for bit; a text that is not of the strict form fails
with the record named and leaves nothing staged; the command line writes the same bytes with and without the flag."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import fastq_cases as fc
from mapper_amd import _capi, api, cli, hostio, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = api.AlignmentParameters()
DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)


def letters(codes):
    return DEC[codes].tobytes()


def fastq_of(reads, name="r%d", quality=b"I"):
    return b"".join(b"@" + (name % i).encode() + b"\n" + letters(r) + b"\n+\n" + quality * len(r) + b"\n" for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def ref():
    return synth.synthetic_reference(30_000, seed=0xFA570)


@pytest.fixture(scope="module")
def db(ref):
    d = api.ReferenceDatabase([("syn", ref)])
    yield d
    d.close()


def lines_of(text):
    return text.count(b"\n") + (0 if text.endswith(b"\n") else 1)


def stage_raw(d, text1, text2=None, records1=None, records2=None, keep=1, spacing=(0.0, 1.0)):
    """xm_batch_stage_fastq on bytes -> the returned arrays (fastq_cases.batch_dict) and the call's times; ValueError with the library's message."""
    b1 = C.create_string_buffer(text1, len(text1))
    b2 = C.create_string_buffer(text2, len(text2)) if text2 is not None else None
    t = _capi.XmFastqText(C.addressof(b1), len(text1), lines_of(text1) // 4 if records1 is None else records1,
                          C.addressof(b2) if b2 is not None else None, len(text2) if b2 is not None else 0,
                          (lines_of(text2) // 4 if records2 is None else records2) if b2 is not None else 0, spacing[0], spacing[1], keep, 0)
    out = C.POINTER(_capi.XmFastqBatch)()
    if d._L.xm_batch_stage_fastq(d._h, C.byref(t), C.byref(out)):
        assert not out
        raise ValueError(d._L.xm_last_error().decode())
    got = fc.batch_dict(out.contents)
    assert out.contents.store is None and out.contents.h2d_ms >= 0 and out.contents.kernel_ms > 0 and out.contents.d2h_ms >= 0
    d._L.xm_fastq_batch_free(out)
    return got


def check_against_reader(d, tmp_path, what, text1, text2=None, keeps=(1, 0)):
    p1 = fc.write(str(tmp_path / "a.fastq"), text1)
    p2 = fc.write(str(tmp_path / "b.fastq"), text2) if text2 is not None else None
    for keep in keeps:
        want = fc.reader_arrays(p1, p2, keep_qualities=bool(keep))
        assert want["num_queries"] == lines_of(text1) // 4
        fc.assert_same_arrays(stage_raw(d, text1, text2, keep=keep, spacing=(100.0, 50.0)), want, (what, keep))


# ---------------------------------------------------------------- the arrays
@pytest.mark.parametrize("name", sorted(fc.rule_texts()))
def test_arrays_equal_the_host_readers(db, tmp_path, name):
    check_against_reader(db, tmp_path, name, fc.rule_texts()[name])


def test_arrays_of_a_pair_equal_the_host_readers(db, tmp_path):
    a, b = fc.pair_texts()
    check_against_reader(db, tmp_path, "pair", a, b)


def record(name_len, seq_len, k=0):
    seq = bytes(b"ACGT"[(k + i * i) % 4] for i in range(seq_len))
    return b"@" + bytes(b"abcdefghij"[(k + i) % 10] for i in range(name_len)) + b"\n" + seq + b"\n+\n" + bytes(33 + (k + i) % 40 for i in range(seq_len)) + b"\n"


def text_of_size(n):
    """A text of exactly n bytes: twenty short records and one whose name fills the rest."""
    body = fc.random_fastq(20, 5)
    rest = n - len(body) - len(record(0, 4))
    assert rest >= 0
    return body + record(rest, 4)


def edge_texts():
    T = _capi.lib().xm_fastq_tile_bytes()
    assert T >= 1024 and T % 16 == 0
    tail = fc.random_fastq(9, 6)
    return {
        "newline_last_byte_of_a_tile": record(T - 2, 40) + tail,                  # the header's newline is byte T - 1
        "newline_first_byte_of_next_tile": record(T - 1, 40) + tail,              # ... byte T
        "sequence_newline_on_both_sides": record(5, T - 8) + record(4, T - 1 - 7) + tail,
        "record_spanning_whole_tiles": fc.random_fastq(3, 8) + record(7, 10_000) + tail,
        "exactly_T": text_of_size(T), "T_minus_1": text_of_size(T - 1), "T_plus_1": text_of_size(T + 1),
        "T_without_final_newline": text_of_size(T + 1)[:-1],
        "records_63": fc.random_fastq(63, 63), "records_64": fc.random_fastq(64, 64), "records_65": fc.random_fastq(65, 65),
        "every_residue": b"".join(record(k % 13, k % 97 + 1, k) for k in range(300)),
        "several_scan_blocks": fc.random_fastq(2500, 9, length=lambda k: 1 + k % 5, name=lambda k: "n" * (k % 3)),  # 5 000 mate slots: two blocks of the offset scan
    }


@pytest.mark.parametrize("name", ["newline_last_byte_of_a_tile", "newline_first_byte_of_next_tile", "sequence_newline_on_both_sides", "record_spanning_whole_tiles", "exactly_T",
                                  "T_minus_1", "T_plus_1", "T_without_final_newline", "records_63", "records_64", "records_65", "every_residue", "several_scan_blocks"])
def test_edges_of_the_line_end_scan(db, tmp_path, name):
    text = edge_texts()[name]
    T = _capi.lib().xm_fastq_tile_bytes()
    if name == "newline_last_byte_of_a_tile":
        assert text[T - 1:T] == b"\n"
    if name == "newline_first_byte_of_next_tile":
        assert text[T:T + 1] == b"\n"
    if name in ("exactly_T", "T_minus_1", "T_plus_1"):
        assert len(text) == {"exactly_T": T, "T_minus_1": T - 1, "T_plus_1": T + 1}[name]
    check_against_reader(db, tmp_path, name, text, keeps=(1,))


def test_edges_in_the_second_file_of_a_pair(db, tmp_path):
    e = edge_texts()
    b = e["every_residue"]
    a = fc.random_fastq(300, 4, length=lambda k: 150 - k % 50, name=lambda k: "p%d/1" % k)
    check_against_reader(db, tmp_path, "pair edges", a, b)


# ---------------------------------------------------------------- what the kernels read
def same_streams(got, want):
    return (np.array_equal(got.int_off, want.int_off) and np.array_equal(got.ints, want.ints) and np.array_equal(got.dbl_off, want.dbl_off)
            and np.array_equal(np.asarray(got.dbls).view(np.int64), np.asarray(want.dbls).view(np.int64)))


def align_both_ways(d, tmp_path, text1, text2=None, spacing=(0.0, 1.0)):
    """(streams of the block the GPU parsed and committed, streams of align_arrays on the host reader's arrays of the same files)"""
    p1 = fc.write(str(tmp_path / "a.fastq"), text1)
    p2 = fc.write(str(tmp_path / "b.fastq"), text2) if text2 is not None else None
    blocks = list(hostio.read_text_blocks(p1, p2, keep_qualities=True, expected_inner=spacing[0], deviation=spacing[1]))
    assert len(blocks) == 1 and blocks[0].num_queries == lines_of(text1) // 4 and blocks[0].longest_line >= 1
    d.stage_fastq(blocks[0])
    d.commit_staged()
    got = d.align_resident(PARAMS)
    staged = [np.array(a) for a in blocks[0].arrays()]
    assert blocks[0].times_ms["kernel"] > 0
    blocks[0].close()
    batches = list(hostio.read_batches(p1, p2, keep_qualities=True, expected_inner=spacing[0], deviation=spacing[1]))
    assert len(batches) == 1
    for a, b in zip(staged, batches[0].arrays()):
        assert np.array_equal(a, b)
    want = d.align_arrays(*batches[0].arrays(), PARAMS)
    batches[0].close()
    return got, want


def test_single_reads_align_as_the_host_readers_arrays_do(db, ref, tmp_path):
    reads = synth.synthetic_single_end(ref, 1000, seed=21)[0]
    got, want = align_both_ways(db, tmp_path, fastq_of(reads))
    assert same_streams(got, want)
    assert sum(1 for q in range(1000) if got.ints[got.int_off[q] + 1] > 0) > 900


def test_pairs_align_as_the_host_readers_arrays_do(db, ref, tmp_path):
    m1, m2 = synth.synthetic_paired_end(ref, 1000, seed=22)[:2]
    got, want = align_both_ways(db, tmp_path, fastq_of(m1, "p%d/1"), fastq_of(m2, "p%d/2"), spacing=(100.0, 50.0))
    assert same_streams(got, want)
    assert sum(1 for q in range(1000) if got.ints[got.int_off[q] + 1] > 0) > 900


def test_collapse_sees_the_same_copies(db, ref, tmp_path):
    reads = list(synth.synthetic_single_end(ref, 900, seed=23)[0])
    reads = reads[:450] + [reads[7]] * 100 + reads[450:]
    c = db.new_context()
    c.set_collapse(True)
    try:
        got, want = align_both_ways(c, tmp_path, fastq_of(reads))
    finally:
        c.close()
    assert same_streams(got, want)
    assert got.copies == want.copies and got.copies >= 100


def test_pile_up_hook_reads_a_staged_block(db, ref, tmp_path):
    reads = synth.synthetic_single_end(ref, 64, seed=24)[0]
    path = fc.write(str(tmp_path / "a.fastq"), fastq_of(reads))
    blocks = list(hostio.read_text_blocks(path, batch_size=40))
    seen = []
    results = list(db.align_stream(iter(blocks), PARAMS, on_aligned=lambda k: seen.append((k, len(blocks[k]), bytes(blocks[k][0][0])))))
    assert [len(r) for r in results] == [40, 24]
    assert seen == [(0, 40, bytes(reads[0])), (1, 24, bytes(reads[40]))]
    for b in blocks:
        b.close()


# ---------------------------------------------------------------- errors
GOOD3 = fc.random_fastq(3, 31)
GOOD2 = fc.random_fastq(2, 32)
GOOD1 = fc.random_fastq(1, 33)
BAD = {
    "empty_line_between_records": (GOOD3 + b"\n" + GOOD2, None, dict(records1=5), "file 1 record 3: an empty line"),
    "fasta_record": (GOOD3 + b">f\nACGT\n+\nIIII\n" + GOOD2, None, {}, "file 1 record 3: a FASTA record"),
    "no_bases": (GOOD3 + b"@r\n\n+\n\n" + GOOD2, None, {}, "file 1 record 3: mate length out of range (1..30000"),
    "too_many_bases": (GOOD3 + b"@r\n" + b"A" * 30001 + b"\n+\nI\n" + GOOD2, None, {}, "file 1 record 3: mate length out of range (1..30000"),
    "records_one_too_few": (GOOD3 + GOOD2, None, dict(records1=4), "file 1 record 4: the text does not hold four lines per record"),
    "records_one_too_many": (GOOD3 + GOOD2, None, dict(records1=6), "file 1 record 5: the text does not hold four lines per record"),
    "pair_of_5_and_4": (GOOD3 + GOOD2, GOOD3 + GOOD1, {}, "file 2 record 4: paired texts have different numbers of records"),
    "second_file_bad": (GOOD3 + GOOD2, GOOD3 + b">f\nACGT\n+\nIIII\n" + GOOD1, {}, "file 2 record 3: a FASTA record"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_errors_name_the_record_and_leave_nothing_staged(db, ref, tmp_path, name):
    text1, text2, kw, message = BAD[name]
    c = db.new_context()
    try:
        with pytest.raises(ValueError) as e:
            stage_raw(c, text1, text2, **kw)
        assert str(e.value).startswith("xm_batch_stage_fastq: " + message), str(e.value)
        with pytest.raises(Exception, match="no staged batch"):
            c.commit_staged()
        reads = synth.synthetic_single_end(ref, 50, seed=25)[0]
        got, want = align_both_ways(c, tmp_path, fastq_of(reads))  # the context then stages and aligns a good block
        assert same_streams(got, want) and sum(1 for q in range(50) if got.ints[got.int_off[q] + 1] > 0) > 40
    finally:
        c.close()


def test_an_error_does_not_disturb_the_resident_batch(db, ref, tmp_path):
    reads = synth.synthetic_single_end(ref, 50, seed=26)[0]
    got, want = align_both_ways(db, tmp_path, fastq_of(reads))
    with pytest.raises(ValueError, match="record 3"):
        stage_raw(db, BAD["fasta_record"][0])
    assert same_streams(db.align_resident(PARAMS), want)


# ---------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def job_files(ref, tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_cli")
    elsewhere = synth.synthetic_reference(5_000, seed=99)  # reads from here align nowhere: the unaligned file gets them, with their qualities
    (d / "ref.fa").write_bytes(b">chrA\n" + letters(ref[:18_000]) + b"\n>chrB\n" + letters(ref[18_000:]) + b"\n")
    single = list(synth.synthetic_single_end(ref, 1900, seed=41)[0]) + list(synth.synthetic_single_end(elsewhere, 100, seed=42)[0])
    m1, m2 = synth.synthetic_paired_end(ref, 1000, seed=43)[:2]
    fc.write(str(d / "se.fq.gz"), fastq_of(single, quality=b"F"), gz=True)
    fc.write(str(d / "se.fq"), fastq_of(single, quality=b"F"))
    fc.write(str(d / "p1.fq"), fastq_of(m1, "p%d/1"))
    fc.write(str(d / "p2.fq"), fastq_of(m2, "p%d/2").replace(b"\n", b"\r\n"))
    return d


def run_job(d, out_dir, args, outputs, flag, in_process=True):
    os.makedirs(out_dir, exist_ok=True)
    argv = ["--reference", str(d / "ref.fa")] + args + [x for name in outputs for x in ("--out-" + name, os.path.join(out_dir, name))] + (["--parse-on-gpu"] if flag else [])
    if in_process:
        log = io.StringIO()
        assert cli.run(argv, out=log) == 0
        text = log.getvalue()
    else:
        r = subprocess.run([sys.executable, "-m", "mapper_amd"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        text = r.stdout
    return {name: open(os.path.join(out_dir, name), "rb").read() for name in outputs}, text[text.index("Statistics"):]


JOBS = {
    "single_gzip_python_m": (lambda d: ["--queries", str(d / "se.fq.gz")], ["sam", "unaligned", "refs-map-count"], False),
    "single_sam_unaligned": (lambda d: ["--queries", str(d / "se.fq.gz")], ["sam", "unaligned"], True),
    "pairs": (lambda d: ["--paired-queries", str(d / "p1.fq"), str(d / "p2.fq"), "--spacing", "100", "50"], ["sam", "unaligned"], True),
    "batches_of_300_two_contexts": (lambda d: ["--queries", str(d / "se.fq"), "--batch-size", "300", "--contexts", "2"], ["sam", "unaligned"], True),
    "mutations": (lambda d: ["--queries", str(d / "se.fq")], ["sam", "mutations"], True),
}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_command_line_writes_the_same_bytes_with_the_flag(job_files, tmp_path, name):
    args, outputs, in_process = JOBS[name]
    without = run_job(job_files, str(tmp_path / "host"), args(job_files), outputs, False, in_process)
    with_flag = run_job(job_files, str(tmp_path / "gpu"), args(job_files), outputs, True, in_process)
    assert with_flag == without
    assert len(without[0]["sam"]) > 100_000 and ("unaligned" not in outputs or name == "pairs" or without[0]["unaligned"].count(b"\n+\n") >= 90)


def test_command_line_passes_the_librarys_message_on(job_files, tmp_path, capsys):
    bad = fc.write(str(tmp_path / "bad.fq"), GOOD3 + b">f\nACGT\n+\nIIII\n" + GOOD2)
    rc = cli.main(["--reference", str(job_files / "ref.fa"), "--queries", bad, "--out-sam", str(tmp_path / "o.sam"), "--parse-on-gpu"])
    err = capsys.readouterr().err
    assert rc == 1 and "file 1 record 3: a FASTA record" in err and "run without --parse-on-gpu" in err
    assert cli.main(["--reference", str(job_files / "ref.fa"), "--queries", bad, "--out-sam", str(tmp_path / "o.sam")]) == 0  # (the host reader takes the file)
