"""The count per combination of contigs without a GPU: the rules the kernels of xm_refs.h apply (mapper_amd/csrc/xm_refs_rules.h, plain C++) and a restatement
of their four stages for one thread, run by tests/refs_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the
host compiler has the runtime), against a recount written in Python (refs_cases.recount: cli.ObjectSink's expression over decoded slices); the seeds of the
GPU tier's cases checked for what that tier asserts of them; the command line's --count-refs-on-gpu: what it accepts and refuses, and the job over a database
that needs no GPU, which must write the file the per-object path writes."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import refs_cases as rc
import sam_cases as sc
import summary_cases as sm
from mapper_amd import cli
from standin_db import StandInDatabase
from test_summary_rules import NoStreamsDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4200]  # the wave, block and scan-block edges (tests/test_gpu_refs_count.py runs the same cases)


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "refs_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/refs_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("refs_rules") / "refs_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + list(args), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def count(program, tmp_path, arrays, num_contigs=rc.NUM_CONTIGS, bits=64):
    """The program's four stages over the streams -> (the folded dict, left-over queries, aligned queries, records), or ("malformed", query)."""
    lines = run(program, "count", sm.write_streams(str(tmp_path / "case.bin"), arrays, num_contigs), str(bits)).decode().split("\n")
    head = lines[0].split()
    if head[0] == "malformed":
        return ("malformed", int(head[1]))
    assert head[0] == "ok"
    nq, aligned, n_records, n_left = (int(x) for x in head[1:])
    assert nq == len(arrays[2]) - 1
    records = []
    for line in lines[1:1 + n_records]:
        f = [int(x) for x in line.split()]
        assert len(f) == 2 + f[1] and 1 <= f[1] <= 8 and f[0] >= 1 and f[2:] == sorted(set(f[2:]))
        records.append((tuple(f[2:]), f[0]))
    assert len({ids for ids, _ in records}) == n_records or bits < 64   # (whole fingerprints: the sets of two records differ)
    leftovers = [[int(x) for x in line.split()] for line in lines[1 + n_records:1 + n_records + n_left]]
    assert all(len(x) >= 1 for x in leftovers) and sum(c for _, c in records) + n_left == aligned
    return rc.fold(records, leftovers), n_left, aligned, records


def check(program, tmp_path, streams, num_contigs=rc.NUM_CONTIGS, bits=64, leftover=None):
    arrays = sm.arrays_of(streams)
    want = rc.recount(arrays, num_contigs)
    got, n_left, aligned, _ = count(program, tmp_path, arrays, num_contigs, bits)
    assert got == want and aligned == sum(want.values())
    if leftover is not None:
        assert n_left == leftover
    return want, n_left


def test_sets_fingerprints_and_comparison(program):
    out = run(program, "fingerprints").split()
    assert out[:2] == [b"fingerprints", b"ok"] and int(out[2]) > 10000 and int(out[3]) > 500, out


@pytest.mark.parametrize("nq", EDGES)
def test_random_streams_at_the_edges_and_what_the_gpu_tier_asserts_of_these_seeds(program, tmp_path, nq):
    streams = rc.random_streams(nq)
    want, _ = check(program, tmp_path, streams, leftover=0)   # whole fingerprints and no wide query: the host is left with nothing
    assert sum(want.values()) >= 0.6 * nq and (nq < 63 or len(want) >= 8)
    if nq >= 63:
        _, n_left = check(program, tmp_path, streams, bits=3)  # at most seven fingerprints for more sets than that: collisions, and the same dict
        assert n_left > 0


def test_one_combination_no_alignment_and_every_query_its_own(program, tmp_path):
    want, _ = check(program, tmp_path, rc.same_combination_case(), leftover=0)
    assert want == {(1, 3): 3360}
    want, _ = check(program, tmp_path, sc.all_unaligned_case(300)[1], leftover=0)
    assert want == {}
    own = rc.own_combination_case()
    want, _ = check(program, tmp_path, own, num_contigs=300, leftover=0)
    assert len(want) == 4097 and set(want.values()) == {1}
    _, n_left = check(program, tmp_path, own, num_contigs=300, bits=3)
    assert n_left >= 4090


def test_sets_of_eight_nine_and_forty_and_the_shapes(program, tmp_path):
    want, _ = check(program, tmp_path, rc.set_sizes_case(), num_contigs=40, leftover=3)   # the two sets of nine and the set of forty
    assert want == {(0,): 2, tuple(range(10, 18)): 3, tuple(range(9)): 2, tuple(range(40)): 1}
    want, _ = check(program, tmp_path, rc.shapes_case(), leftover=0)
    assert want == {(2,): 1, (0, 1): 1, (0, 3): 1, (3,): 1}
    for nq, at in ((65, 63), (300, 256), (4200, 4096)):
        want, _ = check(program, tmp_path, rc.wide_between_unaligned_case(nq, at), num_contigs=64, leftover=1)
        assert want == {tuple(range(40)): 1}
    check(program, tmp_path, sc.shapes_case()[1], leftover=0)


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # what only a SAM record cannot express (tests/test_summary_rules.py)


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_a_malformed_slice_is_reported_with_its_lowest_query(program, tmp_path, name):
    arrays = sc.malformed_cases()[name][1].arrays()
    lowest = 4 if name in SAM_ONLY else 2
    with pytest.raises(rc.Malformed) as e:
        rc.recount(arrays)
    assert e.value.query == lowest
    assert count(program, tmp_path, arrays) == ("malformed", lowest)
    four = sm.first_queries(arrays, 4)
    if name in SAM_ONLY:
        check(program, tmp_path, four)
    else:
        assert count(program, tmp_path, four) == ("malformed", 2)


def test_a_slice_cut_short_anywhere_is_malformed_and_nothing_behind_it_is_read(program, tmp_path):
    streams = sc.one_pair_case()[1]
    out = run(program, "cut", sm.write_streams(str(tmp_path / "pair.bin"), streams.arrays()))
    assert out.split() == [b"cut", b"ok", b"%d" % len(streams.ints), b"%d" % len(streams.dbls)], out


# ---------------------------------------------------------------- the command line

REF, Q, COUNTS = ["--reference", "r.fa"], ["--queries", "q.fq"], ["--out-refs-map-count", "c.txt"]


def test_cli_flag_what_it_makes_possible_and_what_it_excludes():
    sam = ["--out-sam", "o.sam"]
    for more in ([], ["--parse-on-gpu"], sam + ["--format-on-gpu"], ["--results-on-gpu"], sam + ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"],
                 ["--out-mutations", "m.txt", "--results-on-gpu"], ["--out-unaligned", "u.fq", "--parse-on-gpu"], sam):
        for argv in (REF + Q + COUNTS + more + ["--count-refs-on-gpu"], REF + ["--count-refs-on-gpu"] + more + Q + COUNTS):
            o = cli.parse_args(argv)
            assert o["count_refs_on_gpu"] is True and o["out_refs_map_count"] == "c.txt" and not cli.needs_objects(o), argv
    assert cli.needs_objects(cli.parse_args(REF + Q + COUNTS)) and not cli.parse_args(REF + Q + COUNTS).get("count_refs_on_gpu")
    assert cli.needs_objects(cli.parse_args(REF + Q + COUNTS + ["--parse-on-gpu"]))   # (parsed on the host all the same, as before)
    assert not cli.needs_objects(cli.parse_args(REF + Q + ["--no-output"]))
    with pytest.raises(cli.UsageError, match="--count-refs-on-gpu and --per-object exclude each other"):
        cli.parse_args(REF + Q + COUNTS + ["--count-refs-on-gpu", "--per-object"])
    with pytest.raises(cli.UsageError, match="--count-refs-on-gpu has nothing to do without --out-refs-map-count"):
        cli.parse_args(REF + Q + ["--no-output", "--count-refs-on-gpu"])
    with pytest.raises(cli.UsageError, match="--format-on-gpu and --out-mutations exclude each other"):  # (the other rules stand)
        cli.parse_args(REF + Q + COUNTS + sam + ["--count-refs-on-gpu", "--format-on-gpu", "--out-mutations", "m.txt"])
    with pytest.raises(cli.UsageError, match="--results-on-gpu with --out-sam needs --format-on-gpu"):
        cli.parse_args(REF + Q + COUNTS + sam + ["--count-refs-on-gpu", "--results-on-gpu"])


def test_without_the_flag_the_three_refusals_stand():
    with pytest.raises(cli.UsageError, match="--format-on-gpu and --out-refs-map-count exclude each other"):
        cli.parse_args(REF + Q + COUNTS + ["--out-sam", "o.sam", "--format-on-gpu"])
    with pytest.raises(cli.UsageError, match="--results-on-gpu and --out-refs-map-count exclude each other"):
        cli.parse_args(REF + Q + COUNTS + ["--results-on-gpu"])
    with pytest.raises(cli.UsageError, match="--results-on-gpu and --per-object exclude each other"):
        cli.parse_args(REF + Q + COUNTS + ["--results-on-gpu", "--per-object"])


def test_the_key_is_a_set_over_names_and_the_file_is_most_frequent_first(tmp_path):
    assert cli.refs_map_key((2, 0, 1), ["b", "a", "b"]) == ("a", "b") and cli.refs_map_key([1], ["x", "y"]) == ("y",)
    counts = {("chrB",): 7, ("chrA", "chrB"): 7, ("chrA",): 9}
    cli.write_refs_map(str(tmp_path / "direct.txt"), counts)
    sink = cli.ObjectSink(["chrA", "chrB"], count_refs=True)
    sink.refs_map = dict(counts)
    sink.write_refs_map(str(tmp_path / "sink.txt"))
    assert open(tmp_path / "direct.txt").read() == open(tmp_path / "sink.txt").read() == "chrA\t9\nchrA,chrB\t7\nchrB\t7\n"


class CountingDatabase(StandInDatabase):
    """The stand-in as a context that counts: refs_count_last is refs_cases.recount over what the oracle aligned last, while that batch is "resident"."""
    calls = 0

    def align_stream(self, batches, parameters, on_aligned=None):
        for k, r in enumerate(super().align_stream(batches, parameters, on_aligned=None)):
            self.last = (r.ints, r.dbls, r.int_off, r.dbl_off)
            if on_aligned is not None:
                on_aligned(k)
            self.last = None
            yield r

    def refs_count_last(self):
        assert self.last is not None, "the batch is no longer resident"
        CountingDatabase.calls += 1
        return rc.recount(self.last, num_contigs=1 << 30)


class CountingNoStreamsDatabase(NoStreamsDatabase):
    def refs_count_last(self):
        CountingDatabase.calls += 1
        return rc.recount(self.last, num_contigs=1 << 30)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    from mapper_amd import synth
    d = tmp_path_factory.mktemp("count_refs_on_gpu")
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    text = lambda codes: dec[codes].tobytes().decode()  # noqa: E731
    ref = synth.synthetic_reference(20_000, seed=0xEC011)
    elsewhere = synth.synthetic_reference(5_000, seed=99)
    # (two contigs of one name: the count merges them, as the per-object path does)
    (d / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n>chrA\n%s\n" % (text(ref[:8_000]), text(ref[8_000:14_000]), text(ref[14_000:])))
    reads = np.concatenate([synth.synthetic_single_end(ref[:8_000], 70, seed=5)[0], synth.synthetic_single_end(elsewhere, 20, seed=6)[0],
                            synth.synthetic_single_end(ref[8_000:14_000], 50, seed=7)[0], synth.synthetic_single_end(ref[14_000:], 40, seed=8)[0]])
    (d / "se.fq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, text(r), "I" * len(r)) for i, r in enumerate(reads)))
    return ["--reference", str(d / "ref.fa"), "--queries", str(d / "se.fq"), "--batch-size", "64", "--contexts", "1"]


def run_job(argv, database):
    StandInDatabase.opened.clear()
    NoStreamsDatabase.held.clear()
    CountingDatabase.calls = 0
    log = io.StringIO()
    assert cli.run(argv, out=log, open_database=database) == 0
    assert len(StandInDatabase.opened) == 1 and StandInDatabase.opened[0].closed
    return log.getvalue()


def test_the_job_that_counts_on_the_context_writes_what_the_per_object_job_writes(job, tmp_path):
    paths = {k: str(tmp_path / k) for k in ("objects.txt", "objects.sam", "counted.txt", "counted.sam", "resident.txt", "resident.sam", "alone.txt")}
    first = run_job(job + ["--out-refs-map-count", paths["objects.txt"], "--out-sam", paths["objects.sam"]], StandInDatabase)
    want = open(paths["objects.txt"]).read()
    lines = dict(line.split("\t") for line in want.split("\n") if line)
    assert set(lines) == {"chrA", "chrB"} and int(lines["chrA"]) >= 100 and int(lines["chrB"]) >= 45 and CountingDatabase.calls == 0
    # the flag: the streaming path, one count per batch
    log = run_job(job + ["--out-refs-map-count", paths["counted.txt"], "--out-sam", paths["counted.sam"], "--count-refs-on-gpu"], CountingDatabase)
    assert open(paths["counted.txt"]).read() == want and open(paths["counted.sam"]).read() == open(paths["objects.sam"]).read() and log == first
    assert CountingDatabase.calls == 3
    # beside the text and the summary made on the context, with no streams on the host
    log = run_job(job + ["--out-refs-map-count", paths["resident.txt"], "--out-sam", paths["resident.sam"], "--count-refs-on-gpu", "--format-on-gpu", "--results-on-gpu"],
                  CountingNoStreamsDatabase)
    assert open(paths["resident.txt"]).read() == want and open(paths["resident.sam"]).read() == open(paths["objects.sam"]).read() and log == first
    assert CountingDatabase.calls == 3 and len(NoStreamsDatabase.held) == 6 and all(h.closed for h in NoStreamsDatabase.held)
    # the count as the only output
    log = run_job(job + ["--out-refs-map-count", paths["alone.txt"], "--count-refs-on-gpu"], CountingDatabase)
    assert open(paths["alone.txt"]).read() == want and log == first
