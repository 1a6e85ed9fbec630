"""FASTA text for the device parser, without a GPU: the stages the kernels of mapper_amd/csrc/xm_fasta.h run, restated for one thread by
tests/fasta_main.cpp (a stand-alone program built here with g++, with -fsanitize=address,undefined where the host compiler has the runtime) over the rule
functions of xm_fasta_rules.h, against the host reader; what the strict form refuses; the FASTA cutter of libxm_hostio.so, and the FASTQ cutter held against
what it gave before the FASTA one was added (tests/golden/fasta/fastq_cutter_blocks.json); and the command line's --fasta-on-gpu."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fasta_cases as fa
import fastq_cases as fc
import fastq_split_cases as sc
from mapper_amd import cli, hostio

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "fasta_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/fasta_main.cpp")
    out = str(tmp_path_factory.mktemp("fasta") / "fasta_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def stage_arrays(program, split, path1, path2=None, announce=(), keep=True):
    r = subprocess.run([program, "stage", str(split), path1] + ([path2 or "-"] if path2 or announce else []) + [str(x) for x in announce], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    rows = {line.split(" ", 1)[0]: (line.split(" ", 1) + [""])[1] for line in r.stdout.splitlines()}
    if "error" in rows:
        return ("error",) + tuple(int(x) for x in rows["error"].split())
    num = lambda k, t: np.array([int(x) for x in rows[k].split()], dtype=t)  # noqa: E731
    d = {"num_queries": int(rows["nq"]), "mate_count": num("mate_count", np.int32), "mate_offset": num("mate_offset", np.int64), "mate_length": num("mate_length", np.int32),
         "codes": np.frombuffer(bytes.fromhex(rows["codes"]), dtype=np.uint8), "names": bytes.fromhex(rows["names"]), "name_off": num("name_off", np.int64),
         "quals": bytes.fromhex(rows["quals"]), "qual_off": num("qual_off", np.int64), "has_qual": num("has_qual", np.uint8)}
    if not keep:  # (the reader then has no quality arrays at all; a FASTA mate has none to keep either way)
        d["quals"] = d["qual_off"] = d["has_qual"] = None
    return d


# ---------------------------------------------------------------- the stages, one thread
@pytest.mark.parametrize("split", fa.SPLITS)
def test_stages_equal_the_host_reader(program, tmp_path, split):
    for name, text in sorted(fa.texts().items()):
        path = fc.write(str(tmp_path / (name + ".fasta")), text)
        for keep in (True, False):
            want = fa.reader_arrays(path, split=split, keep_qualities=keep, batch_size=5)  # (batches of 5 queries: the reader's sections straddle them)
            fc.assert_same_arrays(stage_arrays(program, split, path, keep=keep), want, (name, split, keep))
        lengths = fa.record_lengths(text)
        assert want["num_queries"] == (sum(len(cli.split_sections(n, split)) for n in lengths) if split else len(lengths)), name
        assert want["mate_length"].sum() == sum(lengths) and (split == 0 or want["mate_length"].max() <= split)
        assert not fa.reader_arrays(path, split=split)["has_qual"].any()


def test_pairs_equal_the_host_reader(program, tmp_path):
    a, b = fa.pair_texts()
    p1, p2 = fc.write(str(tmp_path / "a.fasta"), a), fc.write(str(tmp_path / "b.fasta"), b)
    for keep in (True, False):
        want = fa.reader_arrays(p1, p2, keep_qualities=keep, batch_size=4)
        fc.assert_same_arrays(stage_arrays(program, 0, p1, p2, keep=keep), want, ("pairs", keep))
    assert want["num_queries"] == 6 and set(want["mate_count"]) == {2} and want["mate_length"][-2:].tolist() == [4, 4]


def test_the_words_the_texts_are_made_of():
    """The cases hold what they are named for (so that a change of the helpers cannot empty them)."""
    t = fa.texts()
    assert b"\r\n" in t["crlf"] and b"\n\n" in t["empty_lines"] and t["empty_lines"].endswith(b"\n\n\n") and not t["no_final_newline"].endswith(b"\n")
    assert b"\n@ACGT\n" in t["odd_body_lines"] and b"\n+\n" in t["odd_body_lines"] and b"\n >x\n" in t["odd_body_lines"]
    assert b">\n" in t["names"] and b"\xff" in t["letters"] and b"\n@fq\n" in t["fastq_behind_fasta"]
    assert fa.record_lengths(t["fastq_behind_fasta"]) == [4 + 3 + 8 + 1 + 8, 2 + 4 + 2 + 1 + 2]
    assert fa.record_lengths(t["odd_body_lines"]) == [5 + 1 + 2 + 4 + 5 + 1, 5]
    for w in fa.WIDTHS:
        assert max(len(line) for line in t["width_%d" % w].split(b"\n") if not line.startswith(b">")) == w


# ---------------------------------------------------------------- refusals
GOOD = fa.wrapped(60, [70, 5, 130])
NO_HEADER, NO_BASES, TOO_LONG, RECORD_COUNT, LINE_COUNT = 1, 2, 3, 4, 5
REFUSALS = {
    "first_byte": (b"ACGT\n" + GOOD, 0, ("error", 0, 0, NO_HEADER)),
    "first_byte_blank": (b" >x\nACGT\n" + GOOD, 0, ("error", 0, 0, NO_HEADER)),
    "header_after_header": (GOOD + b">a\n>b\nACGT\n" + GOOD, 0, ("error", 0, 3, NO_BASES)),
    "header_then_blank_lines": (GOOD + b">a\n\n \t\n\r\n" + GOOD, 0, ("error", 0, 3, NO_BASES)),
    "header_last_line": (GOOD + b">a", 0, ("error", 0, 3, NO_BASES)),
    "header_last_line_newline": (GOOD + b">a\n", 7, ("error", 0, 3, NO_BASES)),
    "bases_30001": (GOOD + fa.record(b"long", fa.bases(30_001), 70), 0, ("error", 0, 3, TOO_LONG)),
    "two_bad_records": (b">a\n\n" + GOOD + b">b\n", 0, ("error", 0, 0, NO_BASES)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_file_and_record(program, tmp_path, name):
    text, split, want = REFUSALS[name]
    assert stage_arrays(program, split, fc.write(str(tmp_path / "bad.fasta"), text)) == want


def test_a_record_of_30001_bases_is_31_queries_with_a_split(program, tmp_path):
    path = fc.write(str(tmp_path / "long.fasta"), REFUSALS["bases_30001"][0])
    got = stage_arrays(program, 1000, path)
    fc.assert_same_arrays(got, fa.reader_arrays(path, split=1000), "30001 bases")
    assert got["num_queries"] == 3 + 31 and got["mate_length"].max() == 968
    exact = fc.write(str(tmp_path / "exact.fasta"), fa.record(b"exact", fa.bases(30_000), 60))  # 30 000 bases over 500 lines are a mate
    fc.assert_same_arrays(stage_arrays(program, 0, exact), fa.reader_arrays(exact), "30000 bases")


def test_refusals_in_pairs_and_wrong_counts(program, tmp_path):
    a, b = fa.pair_texts()
    p1 = fc.write(str(tmp_path / "a.fasta"), a)
    bad2 = fc.write(str(tmp_path / "b.fasta"), b.replace(b">p7_2\r\n", b">p7_2\r\n>p7_2b\r\n").replace(b">last2 mate\n\nTTTT\n\n", b""))  # still 6 headers; record 2 of file 2 is empty
    assert stage_arrays(program, 0, p1, bad2) == ("error", 1, 2, NO_BASES)
    bad1 = fc.write(str(tmp_path / "a2.fasta"), a + b"\n>empty")
    bad2 = fc.write(str(tmp_path / "b2.fasta"), b.replace(b">p7_1\r\n", b">p7_1\r\n>p7_1b\r\n"))  # file 1 record 6, file 2 record 1: the lowest (file, record) wins
    assert stage_arrays(program, 0, bad1, bad2) == ("error", 0, 6, NO_BASES)
    records, lines = fa.counts(GOOD)
    good = fc.write(str(tmp_path / "good.fasta"), GOOD)
    assert (records, lines) == (3, 3 + 2 + 1 + 3)
    assert stage_arrays(program, 0, good, announce=(records, lines))["num_queries"] == 3
    assert stage_arrays(program, 0, good, announce=(records + 1, lines)) == ("error", 0, 3, RECORD_COUNT)
    assert stage_arrays(program, 0, good, announce=(records - 1, lines)) == ("error", 0, 2, RECORD_COUNT)
    assert stage_arrays(program, 0, good, announce=(records, lines + 1)) == ("error", 0, 3, LINE_COUNT)
    assert stage_arrays(program, 7, good, announce=(records, lines - 1)) == ("error", 0, 3, LINE_COUNT)


# ---------------------------------------------------------------- the cutter
def blocks_of(path, batch_size, split=0, path2=None):
    out = []
    for b in hostio.read_text_blocks(path, path2, batch_size=batch_size, split=split, fasta=True):
        assert b.fasta and b.split == split and b.paired == bool(path2)
        out.append((b.text(0), b.records(0), b.num_queries, b.longest_line, b.lines(0)) + ((b.text(1), b.records(1), b.lines(1)) if path2 else ()))
        b.close()
    return out


@pytest.mark.parametrize("batch_size", [1, 7, 100_000])
@pytest.mark.parametrize("split", [0, 3, 10])
def test_cutter_keeps_records_whole_and_counts_exactly(tmp_path, batch_size, split):
    t = fa.texts()
    text = t["mixed_widths"] + t["empty_lines"] + t["odd_body_lines"] + t["fastq_behind_fasta"] + t["crlf"] + t["no_final_newline"]
    path = fc.write(str(tmp_path / "reads.fasta"), text)
    blocks = blocks_of(path, batch_size, split)
    assert b"".join(b[0] for b in blocks) == text
    queries = lambda lengths: sum(len(cli.split_sections(n, split)) for n in lengths) if split else len(lengths)  # noqa: E731
    for block, records, nq, longest, lines in blocks:
        assert block.startswith(b">") and (records, lines) == fa.counts(block)  # whole records: a block starts at a header and the next one does too
        lengths = fa.record_lengths(block)
        assert len(lengths) == records and nq == queries(lengths)
        assert nq <= batch_size or records == 1
        assert longest == (min(max(lengths), split) if split else max(lengths))
    assert sum(b[2] for b in blocks) == queries(fa.record_lengths(text)) == fa.reader_arrays(path, split=split)["num_queries"]
    if batch_size == 100_000:
        assert len(blocks) == 1
    for block, nxt in zip(blocks, blocks[1:]):  # a block is as full as it can be: the next record would not have fitted
        assert block[2] + queries(fa.record_lengths(nxt[0])[:1]) > batch_size


def test_a_record_of_more_sections_than_a_batch_stands_alone(tmp_path):
    reads = [20, 3, 50, 4, 9]
    text = b"".join(fa.record(b"r%d" % k, fa.bases(n, k), 8) for k, n in enumerate(reads))
    blocks = blocks_of(fc.write(str(tmp_path / "t.fa"), text), 7, 3)
    assert [(b[1], b[2]) for b in blocks] == [(1, 7), (1, 1), (1, 17), (2, 5)]  # 7 sections fill the first block; the 17 of the 50-base read are a block of their own
    assert b"".join(b[0] for b in blocks) == text


def test_leading_empty_lines_are_dropped_and_other_first_lines_refused(tmp_path):
    text = fa.texts()["width_60"]
    blocks = blocks_of(fc.write(str(tmp_path / "t.fa"), b"\n\r\n\n" + text), 4)
    assert b"".join(b[0] for b in blocks) == text and [b[1] for b in blocks] == [4, 2]
    assert blocks_of(fc.write(str(tmp_path / "e.fa"), b"\n\n\r\n"), 4) == []
    with pytest.raises(hostio.StrictFormError, match=r"bad.fa: line 3 is neither a FASTA nor a FASTQ header"):
        blocks_of(fc.write(str(tmp_path / "bad.fa"), b"\n\n >x\nACGT\n"), 4)
    with pytest.raises(hostio.StrictFormError, match=r"fq.fa: line 2 is a FASTQ header where FASTA records were announced"):
        blocks_of(fc.write(str(tmp_path / "fq.fa"), b"\n@x\nACGT\n+\nIIII\n"), 4)
    with pytest.raises(OSError, match="0 .. 30000"):
        blocks_of(str(tmp_path / "t.fa"), 4, split=30_001)
    with pytest.raises(ValueError, match="single reads"):
        list(hostio.read_text_blocks(str(tmp_path / "t.fa"), str(tmp_path / "t.fa"), split=10, fasta=True))


@pytest.mark.parametrize("batch_size", [1, 4, 100])
def test_pairs_are_cut_in_step(tmp_path, batch_size):
    a, b = fa.pair_texts()
    p1, p2 = fc.write(str(tmp_path / "a.fasta"), b"\n" + a), fc.write(str(tmp_path / "b.fasta"), b)
    blocks = blocks_of(p1, batch_size, path2=p2)
    assert b"".join(x[0] for x in blocks) == a and b"".join(x[5] for x in blocks) == b
    for text1, records1, nq, _, lines1, text2, records2, lines2 in blocks:
        assert records1 == records2 == nq <= batch_size and (records1, lines1) == fa.counts(text1) and (records2, lines2) == fa.counts(text2)
    assert sum(x[1] for x in blocks) == 6


def test_pairs_of_different_counts_are_refused_with_the_line(tmp_path):
    a, b = fa.pair_texts()
    p1 = fc.write(str(tmp_path / "a.fasta"), a)
    shorter = fc.write(str(tmp_path / "b.fasta"), b[:b.index(b">last2")])
    lines = fa.counts(b[:b.index(b">last2")])[1]
    for batch_size in (2, 100):
        with pytest.raises(hostio.StrictFormError, match=r"different numbers of reads: .*a.fasta, .*b.fasta \(.*b.fasta ends at line %d\)" % lines):
            blocks_of(p1, batch_size, path2=shorter)
    with pytest.raises(hostio.StrictFormError, match=r"different numbers of reads: .*b.fasta, .*a.fasta \(.*b.fasta ends at line %d\)" % lines):
        blocks_of(shorter, 100, path2=p1)


def test_gz_input_and_the_first_header_byte(tmp_path):
    text = fa.texts()["mixed_widths"]
    plain, gz = fc.write(str(tmp_path / "t.fa"), text), fc.write(str(tmp_path / "t.fa.gz"), b"\n" + text, gz=True)
    assert blocks_of(gz, 7, 10) == blocks_of(plain, 7, 10) and len(blocks_of(gz, 7, 10)) > 5
    assert hostio.first_header_byte(plain) == b">" == hostio.first_header_byte(gz)
    assert hostio.first_header_byte(fc.write(str(tmp_path / "q.fq"), b"\r\n\n" + fc.random_fastq(2, 1))) == b"@"
    assert hostio.first_header_byte(fc.write(str(tmp_path / "q.fq.gz"), fc.random_fastq(2, 1), gz=True)) == b"@"
    assert hostio.first_header_byte(fc.write(str(tmp_path / "empty"), b"\n\n")) == b"" == hostio.first_header_byte(fc.write(str(tmp_path / "empty2"), b""))
    with pytest.raises(hostio.StrictFormError, match="x.fa: line 2 is neither a FASTA nor a FASTQ header"):
        hostio.first_header_byte(fc.write(str(tmp_path / "x.fa"), b"\nACGT\n"))
    with pytest.raises(OSError, match="cannot open"):
        hostio.first_header_byte(str(tmp_path / "missing.fa"))


def fastq_cutter_cases():
    """name -> (text, batch_size, split): the FASTQ texts of the existing case files, cut as tests/test_fastq_text.py and tests/test_fastq_split.py cut them."""
    cases = {}
    for name, text in sorted(fc.rule_texts().items()):
        for batch_size in (1, 3, 1000):
            cases["%s/%d/0" % (name, batch_size)] = (text, batch_size, 0)
    for split in (3, 10):
        text = fc.random_fastq(40, 7, length=lambda k: 1 + (k * 7) % 45) + sc.edge_text(split) + fc.rule_texts()["rules_no_final_newline"]
        for batch_size in (1, 7, 1000):
            cases["edges/%d/%d" % (batch_size, split)] = (text, batch_size, split)
            cases["edges/%d/0" % batch_size] = (text, batch_size, 0)
    cases["trailing_empty_lines/7/0"] = (fc.random_fastq(20, 3) + b"\n\r\n\n", 7, 0)
    cases["crlf/5/0"] = (fc.random_fastq(20, 4, crlf=True), 5, 0)
    return cases


def fastq_cutter_blocks(tmp_path):
    out = {}
    for name, (text, batch_size, split) in sorted(fastq_cutter_cases().items()):
        path = fc.write(str(tmp_path / "t.fastq"), text)
        out[name] = [[hashlib.sha256(b.text(0)).hexdigest()[:16], b.records(0), b.num_queries, b.longest_line] for b in hostio.read_text_blocks(path, batch_size=batch_size, split=split)]
    return out


def test_the_fastq_cutter_is_what_it_was(tmp_path):
    """xmio_text_open / xmio_text_open_split blocks against the ones recorded from the library before the FASTA cutter was added."""
    with open(os.path.join(HERE, "golden", "fasta", "fastq_cutter_blocks.json")) as f:
        want = json.load(f)
    got = fastq_cutter_blocks(tmp_path)
    assert sorted(got) == sorted(want) and len(want) > 20
    for name in sorted(want):
        assert got[name] == want[name], name
    path = fc.write(str(tmp_path / "t.fastq"), fc.random_fastq(9, 2))
    for b in hostio.read_text_blocks(path, batch_size=4):  # what the blocks newly carry
        assert not b.fasta and b.lines(0) == 4 * b.records(0) and b.lines(1) == 0


# ---------------------------------------------------------------- the command line
def test_cli_flag_rules():
    base = ["--reference", "r.fa", "--out-sam", "o.sam", "--queries", "q.fa"]
    o = cli.parse_args(base + ["--parse-on-gpu", "--fasta-on-gpu"])
    assert o["parse_on_gpu"] is True and o["fasta_on_gpu"] is True
    assert not cli.parse_args(base + ["--parse-on-gpu"]).get("fasta_on_gpu")
    with pytest.raises(cli.UsageError, match="--fasta-on-gpu needs --parse-on-gpu"):
        cli.parse_args(base + ["--fasta-on-gpu"])
    with pytest.raises(cli.UsageError, match="--per-object"):
        cli.parse_args(base + ["--parse-on-gpu", "--fasta-on-gpu", "--per-object"])
    split = ["--reference", "r.fa", "--out-sam", "o.sam", "--split-queries-past-size", "100", "--queries", "q.fa"]
    with pytest.raises(cli.UsageError) as e:  # a split size still needs --split-on-gpu, in the words it had
        cli.parse_args(split + ["--parse-on-gpu", "--fasta-on-gpu"])
    assert str(e.value) == "--parse-on-gpu is not supported with --split-queries-past-size (the sections are cut by the host reader)"
    o = cli.parse_args(split + ["--out-refs-map-count", "c.txt", "--out-unaligned", "u.fa", "--parse-on-gpu", "--fasta-on-gpu", "--split-on-gpu", "--format-on-gpu", "--results-on-gpu",
                                "--count-refs-on-gpu"])
    assert all(o[k] for k in ("parse_on_gpu", "fasta_on_gpu", "split_on_gpu", "format_on_gpu", "results_on_gpu", "count_refs_on_gpu"))
    o = cli.parse_args(["--reference", "r.fa", "--paired-queries", "a.fa", "b.fa", "--spacing", "100", "50", "--out-mutations", "m.txt", "--parse-on-gpu", "--fasta-on-gpu", "--results-on-gpu"])
    assert o["fasta_on_gpu"] is True and o["paired"][0][:2] == ("a.fa", "b.fa")
