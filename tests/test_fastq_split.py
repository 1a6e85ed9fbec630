"""Long reads cut into sections while FASTQ text is parsed, without a GPU: the section rule of mapper_amd/csrc/xm_fastq_rules.h against
cli.split_sections; the stages the kernels of xm_fastq.h run with a split size, restated for one thread by tests/fastq_split_main.cpp (a stand-alone program
built here with g++, with -fsanitize=address,undefined where the host compiler has the runtime) over the same rule functions, against the host reader; the
cutter of libxm_hostio.so with a split size; and the command line's --split-on-gpu."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastq_cases as fc
import fastq_split_cases as sc
from mapper_amd import cli, hostio

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "fastq_split_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/fastq_split_main.cpp")
    out = str(tmp_path_factory.mktemp("fastq_split") / "fastq_split_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


# ---------------------------------------------------------------- the rule
def check_partition(length, split, sections):
    assert sections[0][0] == 0 and sections[-1][1] == length
    assert all(a[1] == b[0] for a, b in zip(sections, sections[1:]))
    assert all(0 < e - s <= split for s, e in sections)


def test_rule_equals_split_sections_on_the_grid(program):
    rows = run(program, "grid", 200, 50)
    assert len(rows) == 200 * 50
    for row in rows:
        v = [int(x) for x in row.split()]
        length, split, sections = v[0], v[1], list(zip(v[2::2], v[3::2]))
        check_partition(length, split, sections)
        assert sections == cli.split_sections(length, split), (length, split)


@pytest.mark.parametrize("length,split", [(30_000, 30_000), (30_001, 30_000), (2 ** 30 - 1, 30_000)])
def test_rule_equals_split_sections_at_the_limits(program, length, split):
    rows = run(program, "rule", length, split)
    want = cli.split_sections(length, split)
    assert rows[0] == "count %d" % len(want)
    sections = [tuple(int(x) for x in row.split()[1:]) for row in rows[1:]]
    check_partition(length, split, sections)
    assert sections == want
    assert len(want) == {30_000: 1, 30_001: 2, 2 ** 30 - 1: 35792}[length]


def test_rule_with_a_section_per_base_of_the_longest_text(program):
    """(2^30 - 1, 1): 2^30 - 1 sections, where length * (k + 1) is largest.  cli.split_sections would build a list of 2^30 tuples, so the Python rule is its
    expression at the sections asked for; the program checks the sections themselves - the first and the last 2^20 as a run, and two neighbours at every
    1021st between them (section k + 1 starts with the expression section k ends with, so a gap can only come from the arithmetic at that k)."""
    length, split = 2 ** 30 - 1, 1
    num = (length - 1) // split + 1
    ks = sorted({0, 1, 2, 1000, num // 3, num // 2, 2 ** 29, 2 ** 29 + 1, num - 3, num - 2, num - 1})
    rows = run(program, "rule", length, split, *ks)
    assert rows[0] == "count %d" % num, rows[:3]
    assert [tuple(int(x) for x in row.split()) for row in rows[1:]] == [(k, length * k // num, length * (k + 1) // num) for k in ks]
    assert all(int(row.split()[2]) - int(row.split()[1]) == 1 for row in rows[1:])


# ---------------------------------------------------------------- the stages, one thread
def stage_arrays(program, path, split):
    rows = run(program, "stage", path, split)
    rows = {line.split(" ", 1)[0]: (line.split(" ", 1) + [""])[1] for line in rows}
    if "error" in rows:
        return ("error",) + tuple(int(x) for x in rows["error"].split())
    num = lambda k, t: np.array([int(x) for x in rows[k].split()], dtype=t)  # noqa: E731
    return {"num_queries": int(rows["nq"]), "mate_count": num("mate_count", np.int32), "mate_offset": num("mate_offset", np.int64), "mate_length": num("mate_length", np.int32),
            "codes": np.frombuffer(bytes.fromhex(rows["codes"]), dtype=np.uint8), "names": bytes.fromhex(rows["names"]), "name_off": num("name_off", np.int64),
            "quals": bytes.fromhex(rows["quals"]), "qual_off": num("qual_off", np.int64), "has_qual": num("has_qual", np.uint8)}


@pytest.mark.parametrize("split", sc.SPLITS)
def test_stages_equal_the_host_reader(program, tmp_path, split):
    for name, text in sorted(sc.texts(split).items()):
        path = fc.write(str(tmp_path / (name + ".fastq")), text)
        want = sc.reader_arrays(path, split, batch_size=5)  # (batches of 5 queries: the reader's sections straddle them)
        assert want["num_queries"] == sum(len(cli.split_sections(n, split)) for n in sc.sequence_lengths(text)), name
        assert not want["has_qual"].any() and want["quals"] == b"" and set(want["mate_count"]) == {1}
        fc.assert_same_arrays(stage_arrays(program, path, split), want, (name, split))
        if name == "edge_lengths":
            assert sc.edge_lengths(split)[-1] == 10 * split + 3 and want["mate_length"].max() == split


def test_a_record_longer_than_a_mate_is_cut_and_the_other_refusals_stay(program, tmp_path):
    good = fc.random_fastq(3, 1)
    long_read = b"@long\n" + sc.read_of(30_001) + b"\n+\nI\n"
    path = fc.write(str(tmp_path / "long.fastq"), good + long_read)
    got = stage_arrays(program, path, 1000)
    fc.assert_same_arrays(got, sc.reader_arrays(path, 1000), "30001 bases")
    assert got["num_queries"] == 3 + 31 and got["mate_length"].max() == 968
    for bad, code in ((b"\n\n\n\n", 1), (b">fasta\nACGT\n+\nIIII\n", 2), (b"x@r\nACGT\n+\nIIII\n", 3), (b"@r\n \t\n+\n\n", 4)):
        assert stage_arrays(program, fc.write(str(tmp_path / "bad.fastq"), good + bad + good), 3) == ("error", 0, 3, code)
    assert stage_arrays(program, fc.write(str(tmp_path / "bad.fastq"), good + b"@r\nACGT\n"), 3)[3] == 6


# ---------------------------------------------------------------- the cutter
def blocks_of(path, batch_size, split):
    out = []
    for b in hostio.read_text_blocks(path, batch_size=batch_size, split=split):
        assert b.split == split and not b.paired
        out.append((b.text(0), b.records(0), b.num_queries, b.longest_line))
        b.close()
    return out


@pytest.mark.parametrize("batch_size", [1, 7, 1000])
@pytest.mark.parametrize("split", [3, 10])
def test_cutter_counts_sections_and_keeps_records_whole(tmp_path, batch_size, split):
    text = fc.random_fastq(40, 7, length=lambda k: 1 + (k * 7) % 45) + sc.edge_text(split) + fc.rule_texts()["rules_no_final_newline"]
    path = fc.write(str(tmp_path / "reads.fastq"), text)
    blocks = blocks_of(path, batch_size, split)
    assert b"".join(b[0] for b in blocks) == text
    for i, (t, records, nq, longest) in enumerate(blocks):
        assert t.count(b"\n") == 4 * records - (1 if i == len(blocks) - 1 else 0)  # whole records (the file lacks its final newline)
        assert nq == sum(len(cli.split_sections(n, split)) for n in sc.sequence_lengths(t))
        assert nq <= batch_size or records == 1
        assert 1 <= longest <= split
    want = sum(len(cli.split_sections(n, split)) for n in sc.sequence_lengths(text))
    assert sum(b[2] for b in blocks) == want == sc.reader_arrays(path, split)["num_queries"]
    if batch_size == 1:
        assert all(b[1] == 1 for b in blocks)
    if batch_size == 1000:
        assert len(blocks) == 1
    # a block is as full as it can be: the next record would not have fitted
    for (t, records, nq, _), nxt in zip(blocks, blocks[1:]):
        assert nq + len(cli.split_sections(sc.sequence_lengths(nxt[0])[0], split)) > batch_size


def test_a_record_of_more_sections_than_a_batch_stands_alone(tmp_path):
    reads = [20, 3, 50, 4, 9]
    text = b"".join(b"@r%d\n" % k + sc.read_of(n, k) + b"\n+\n" + b"I" * n + b"\n" for k, n in enumerate(reads))
    blocks = blocks_of(fc.write(str(tmp_path / "t.fq"), text), 7, 3)
    assert [(b[1], b[2]) for b in blocks] == [(1, 7), (1, 1), (1, 17), (2, 5)]  # 7 sections fill the first block; the 17 of the 50-base read are a block of their own
    assert b"".join(b[0] for b in blocks) == text
    for tail in (b"\n\n", b""):  # trailing empty lines are dropped; a last record without its newline is a record
        blocks = blocks_of(fc.write(str(tmp_path / "t.fq"), text[:-1] + tail), 7, 3)
        assert [(b[1], b[2]) for b in blocks] == [(1, 7), (1, 1), (1, 17), (2, 5)] and b"".join(b[0] for b in blocks) == text[:-1] + tail[:1]


def test_cutter_without_a_split_is_what_it_was(tmp_path):
    text = fc.random_fastq(50, 7)
    path = fc.write(str(tmp_path / "reads.fastq"), text)
    blocks = [(b.text(0), b.records(0), b.num_queries, b.longest_line, b.split) for b in hostio.read_text_blocks(path, batch_size=7)]
    assert [b[1] for b in blocks] == [7] * 7 + [1] and all(b[2] == b[1] and b[4] == 0 for b in blocks) and max(b[3] for b in blocks) == 50
    with pytest.raises(ValueError, match="single reads"):
        list(hostio.read_text_blocks(path, path, split=10))
    with pytest.raises(OSError, match="1 .. 30000"):
        list(hostio.read_text_blocks(path, split=30_001))


# ---------------------------------------------------------------- the command line
def test_cli_flag_rules():
    base = ["--reference", "r.fa", "--out-sam", "o.sam"]
    split = ["--split-queries-past-size", "100", "--queries", "q.fq"]
    o = cli.parse_args(base + split + ["--parse-on-gpu", "--split-on-gpu"])
    assert o["parse_on_gpu"] is True and o["split_on_gpu"] is True and o["queries"] == [("q.fq", 100)]
    with pytest.raises(cli.UsageError) as e:  # without the new flag: the message it was
        cli.parse_args(base + split + ["--parse-on-gpu"])
    assert str(e.value) == "--parse-on-gpu is not supported with --split-queries-past-size (the sections are cut by the host reader)"
    with pytest.raises(cli.UsageError, match="--split-on-gpu needs --parse-on-gpu"):
        cli.parse_args(base + split + ["--split-on-gpu"])
    with pytest.raises(cli.UsageError, match="--split-on-gpu has nothing to do without --split-queries-past-size"):
        cli.parse_args(base + ["--queries", "q.fq", "--parse-on-gpu", "--split-on-gpu"])
    with pytest.raises(cli.UsageError, match="at most 30000"):
        cli.parse_args(base + ["--split-queries-past-size", "30001", "--queries", "q.fq", "--parse-on-gpu", "--split-on-gpu"])
    with pytest.raises(cli.UsageError, match="--per-object"):
        cli.parse_args(base + split + ["--parse-on-gpu", "--split-on-gpu", "--per-object"])
    assert not cli.parse_args(base + split).get("split_on_gpu")
    # beside the other device stages
    o = cli.parse_args(["--reference", "r.fa"] + split + ["--out-sam", "o.sam", "--out-refs-map-count", "c.txt", "--out-unaligned", "u.fq", "--parse-on-gpu", "--split-on-gpu",
                                                         "--format-on-gpu", "--results-on-gpu", "--count-refs-on-gpu", "--contexts", "2"])
    assert all(o[k] for k in ("parse_on_gpu", "split_on_gpu", "format_on_gpu", "results_on_gpu", "count_refs_on_gpu"))
    assert cli.parse_args(["--reference", "r.fa"] + split + ["--out-mutations", "m.txt", "--parse-on-gpu", "--split-on-gpu", "--results-on-gpu"])["split_on_gpu"] is True
