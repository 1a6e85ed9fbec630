"""FASTQ as text, without a GPU: the rules the device parser applies (mapper_amd/csrc/xm_fastq_rules.h, plain C++ that the kernels of xm_fastq.h call) run by
tests/fastq_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the runtime), against the
host reader, which defines what a record means; the cutter of libxm_hostio.so (hostio.read_text_blocks); and the command line's --parse-on-gpu."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastq_cases as fc
from mapper_amd import cli, hostio

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "fastq_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/fastq_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("fastq_rules") / "fastq_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def rules_arrays(program, *paths):
    """The program's output -> the dict fastq_cases.batch_dict gives, or ("error", file, record, code)."""
    r = subprocess.run([program] + list(paths), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    rows = {line.split(" ", 1)[0]: (line.split(" ", 1) + [""])[1] for line in r.stdout.splitlines()}
    if "error" in rows:
        return ("error",) + tuple(int(x) for x in rows["error"].split())
    num = lambda k, t: np.array([int(x) for x in rows[k].split()], dtype=t)  # noqa: E731
    return {"num_queries": int(rows["nq"]), "mate_count": num("mate_count", np.int32), "mate_offset": num("mate_offset", np.int64), "mate_length": num("mate_length", np.int32),
            "codes": np.frombuffer(bytes.fromhex(rows["codes"]), dtype=np.uint8), "names": bytes.fromhex(rows["names"]), "name_off": num("name_off", np.int64),
            "quals": bytes.fromhex(rows["quals"]), "qual_off": num("qual_off", np.int64), "has_qual": num("has_qual", np.uint8)}


@pytest.mark.parametrize("name", sorted(fc.rule_texts()))
def test_rules_equal_the_host_reader(program, tmp_path, name):
    path = fc.write(str(tmp_path / (name + ".fastq")), fc.rule_texts()[name])
    want = fc.reader_arrays(path)
    assert want["num_queries"] == {"rules_no_final_newline": 7, "rules_final_newline": 7, "crlf_only": 4, "one_record": 1}[name]  # (the reader took every record)
    fc.assert_same_arrays(rules_arrays(program, path), want, name)


def test_rules_equal_the_host_reader_on_a_pair(program, tmp_path):
    a, b = fc.pair_texts()
    pa, pb = fc.write(str(tmp_path / "a.fastq"), a), fc.write(str(tmp_path / "b.fastq"), b)
    want = fc.reader_arrays(pa, pb)
    assert want["num_queries"] == 7 and set(want["mate_count"]) == {2}
    fc.assert_same_arrays(rules_arrays(program, pa, pb), want, "pair")


def test_code_table_is_the_readers(program, tmp_path):
    """All 256 bytes but the line end as bases of one record ('\\r' inside the line: only a trailing one is trimmed)."""
    seq = bytes(b for b in range(256) if b != 0x0A and b != 0x0D) + b"\rA"
    seq = b"A" + seq  # (no blank in front, which would be trimmed)
    path = fc.write(str(tmp_path / "bytes.fastq"), b"@all\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    want = fc.reader_arrays(path)
    assert want["mate_length"][0] == len(seq)
    fc.assert_same_arrays(rules_arrays(program, path), want, "all bytes")


def test_strict_form_names_the_first_offender(program, tmp_path):
    good = fc.random_fastq(3, 1)
    for bad, code in ((b"\n", 1), (b">fasta\nACGT\n+\nIIII\n", 2), (b"x@r\nACGT\n+\nIIII\n", 3), (b"@r\n \t\n+\n\n", 4), (b"@r\n" + b"A" * 30001 + b"\n+\nI\n", 5)):
        text = good + (bad + b"\n\n\n" if bad == b"\n" else bad) + good
        assert rules_arrays(program, fc.write(str(tmp_path / "bad.fastq"), text)) == ("error", 0, 3, code)
    assert rules_arrays(program, fc.write(str(tmp_path / "bad.fastq"), good + b"@r\nACGT\n"))[3] == 6
    ok = rules_arrays(program, fc.write(str(tmp_path / "edge.fastq"), b"@r\n" + b"A" * 30000 + b"\n+\nI\n"))
    assert ok["mate_length"][0] == 30000


# ---------------------------------------------------------------- the cutter
def blocks_of(path1, path2=None, batch_size=1000):
    out = []
    for b in hostio.read_text_blocks(path1, path2, batch_size=batch_size):
        out.append((b.text(0), b.records(0), b.text(1) if path2 else b"", b.records(1) if path2 else 0, b.longest_line, b.num_queries))
        b.close()
    return out


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("batch_size", [1, 7, 1000])
def test_blocks_join_back_to_the_file(tmp_path, batch_size, gz):
    text = fc.random_fastq(50, 7, crlf=batch_size == 7)
    path = fc.write(str(tmp_path / ("reads.fastq" + (".gz" if gz else ""))), text, gz=gz)
    blocks = blocks_of(path, batch_size=batch_size)
    assert b"".join(b[0] for b in blocks) == text
    assert [b[1] for b in blocks] == [min(batch_size, 50 - s) for s in range(0, 50, batch_size)]
    assert all(b[5] == b[1] and b[0].count(b"\n") == 4 * b[1] for b in blocks)
    longest = max(int(b.mate_length.max()) for b in hostio.read_batches(path))
    assert max(b[4] for b in blocks) >= longest and all(b[4] <= longest + 1 for b in blocks)  # (+1: the '\r' of a CRLF file is part of the line)


def test_pair_blocks_stay_in_step(tmp_path):
    a = fc.random_fastq(50, 11, length=lambda k: 20 + k % 31)
    b = fc.random_fastq(50, 12, length=lambda k: 150 - 2 * (k % 40), name=lambda k: "a_much_longer_name_%d/2" % k)
    pa, pb = fc.write(str(tmp_path / "a.fq"), a), fc.write(str(tmp_path / "b.fq.gz"), b, gz=True)
    for batch_size in (1, 7, 1000):
        blocks = blocks_of(pa, pb, batch_size)
        assert b"".join(x[0] for x in blocks) == a and b"".join(x[2] for x in blocks) == b
        assert all(x[1] == x[3] == x[5] and x[2].count(b"\n") == 4 * x[3] for x in blocks) and sum(x[1] for x in blocks) == 50
        assert max(x[4] for x in blocks) == 150


def test_large_blocks_hand_over_the_buffer(tmp_path):
    """A block of most of the source's buffer takes the buffer instead of a copy, the source goes on in another one, and freed buffers go round: 25 MB of
    fixed-width records in blocks of 22 MB and 3 MB, read three times over (the later passes start in the buffers the first one left)."""
    n, length = 80_000, 150
    rng = np.random.default_rng(5)
    head = np.frombuffer(b"@r%07d\n" % 0, dtype=np.uint8)
    rows = np.empty((n, len(head) + 2 * length + 4), dtype=np.uint8)
    rows[:, :len(head)] = head
    for k in range(7):
        rows[:, 2 + k] = 48 + (np.arange(n) // 10 ** (6 - k)) % 10
    rows[:, len(head):len(head) + length] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, length))]
    rows[:, len(head) + length:len(head) + length + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rows[:, len(head) + length + 3:-1] = 70
    rows[:, -1] = 10
    text = rows.tobytes()
    path = fc.write(str(tmp_path / "big.fq"), text)
    for _ in range(3):
        blocks = blocks_of(path, batch_size=70_000)
        assert [b[1] for b in blocks] == [70_000, 10_000] and all(b[4] == length for b in blocks)
        assert blocks[0][0] + blocks[1][0] == text
    held = []  # blocks that are alive at the same time own different buffers
    for b in hostio.read_text_blocks(path, batch_size=35_000):
        held.append(b)
    assert b"".join(b.text(0) for b in held) == text and [b.records(0) for b in held] == [35_000, 35_000, 10_000]
    for b in held:
        b.close()


def test_last_record_without_newline_and_trailing_empty_lines(tmp_path):
    text = fc.random_fastq(5, 3)
    for tail in (b"\n\n\r\n", b"\n" * 9, b""):
        blocks = blocks_of(fc.write(str(tmp_path / "t.fq"), text + tail), batch_size=2)
        assert b"".join(b[0] for b in blocks) == text and [b[1] for b in blocks] == [2, 2, 1]
    blocks = blocks_of(fc.write(str(tmp_path / "t.fq"), text[:-1] + b"\r"), batch_size=1000)  # no final newline
    assert blocks[0][0] == text[:-1] + b"\r" and blocks[0][1] == 5
    blocks = blocks_of(fc.write(str(tmp_path / "t.fq"), text[:-1]), batch_size=4)
    assert [b[1] for b in blocks] == [4, 1] and blocks[1][0] == text[len(blocks[0][0]):-1]


def test_file_that_ends_inside_a_record_names_the_line(tmp_path):
    text = fc.random_fastq(5, 3) + b"@cut\nACGT\n"
    with pytest.raises(hostio.StrictFormError) as e:
        blocks_of(fc.write(str(tmp_path / "cut.fq"), text), batch_size=3)
    assert "t.fq" in str(e.value) and "line 22" in str(e.value) and "2 of the 4 lines" in str(e.value)


def test_pair_files_of_5_and_6_records_fail_with_the_readers_message(tmp_path):
    pa, pb = fc.write(str(tmp_path / "a.fq"), fc.random_fastq(5, 1)), fc.write(str(tmp_path / "b.fq"), fc.random_fastq(6, 2))
    for first, second in ((pa, pb), (pb, pa)):
        for batch_size in (2, 5, 1000):
            with pytest.raises(ValueError, match="paired query files have different numbers of reads"):
                blocks_of(first, second, batch_size)
    with pytest.raises(ValueError, match="paired query files have different numbers of reads"):  # (the reader's own words)
        list(hostio.read_batches(pa, pb))


# ---------------------------------------------------------------- the command line
def test_cli_flag_and_what_it_excludes():
    base = ["--reference", "r.fa", "--out-sam", "o.sam"]
    assert cli.parse_args(base + ["--queries", "q.fq", "--parse-on-gpu"])["parse_on_gpu"] is True
    assert not cli.parse_args(base + ["--queries", "q.fq"]).get("parse_on_gpu")
    assert cli.parse_args(base + ["--paired-queries", "a.fq", "b.fq", "--spacing", "100", "50", "--parse-on-gpu"])["parse_on_gpu"] is True
    with pytest.raises(cli.UsageError, match="--per-object"):
        cli.parse_args(base + ["--queries", "q.fq", "--parse-on-gpu", "--per-object"])
    with pytest.raises(cli.UsageError, match="--split-queries-past-size"):
        cli.parse_args(base + ["--parse-on-gpu", "--split-queries-past-size", "100", "--queries", "q.fq"])
