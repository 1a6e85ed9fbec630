"""The consumers of the result walk agree, without a GPU: the SAM records, the batch summary and the reference sets are visitors of one walk of a query's
slice (mapper_amd/csrc/xm_result_walk.h), so they call the same slices malformed - but for what only a SAM record cannot express, which the SAM visitor
alone refuses.  tests/result_walk_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the
runtime), runs the three side by side over the cases of sam_cases.py."""
import os
import shutil
import subprocess

import pytest

import sam_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # what only a SAM record cannot express (tests/test_summary_rules.py)


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "result_walk_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/result_walk_main.cpp")
    out = str(tmp_path_factory.mktemp("result_walk") / "result_walk_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + list(args), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.decode().split("\n")[:-1]


def verdicts(program, tmp_path, batch, streams):
    """-> per query (sam, summary, refs): whether each walk takes the slice."""
    lines = run(program, "verdicts", sc.write_case(str(tmp_path / "case.bin"), batch, streams))
    assert len(lines) == batch.num_queries
    return [tuple(w == "1" for w in line.split()) for line in lines]


def test_every_shape_is_taken_by_all_three(program, tmp_path):
    batch, streams = sc.shapes_case()
    assert verdicts(program, tmp_path, batch, streams) == [(True, True, True)] * 25


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_streams_are_taken_by_all_three(program, tmp_path, seed):
    batch, streams = sc.random_case(seed, 400)
    assert verdicts(program, tmp_path, batch, streams) == [(True, True, True)] * 400


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_the_verdicts_on_a_malformed_case(program, tmp_path, name):
    """Query 2 is malformed for the SAM records and query 4 for everyone; what the summary rejects in query 2 the reference sets reject too, and what only a
    SAM record cannot express both take."""
    batch, streams, query = sc.malformed_cases()[name]
    got = verdicts(program, tmp_path, batch, streams)
    assert query == 2 and len(got) == 5
    for q, (sam, summary, refs) in enumerate(got):
        assert summary == refs, q
        if name not in SAM_ONLY:
            assert sam == summary, q
    first = lambda k: min(q for q in range(5) if not got[q][k])  # noqa: E731
    if name in SAM_ONLY:
        assert (first(0), first(1), first(2)) == (2, 4, 4)
        assert [sam == summary for sam, summary, _ in got] == [True, True, False, True, True]
    else:
        assert (first(0), first(1), first(2)) == (2, 2, 2)


def test_every_cut_of_a_slice_gets_one_verdict(program, tmp_path):
    """The pair's slice cut short at every int and at every double (each cut in a heap block of its own size: the sanitizer build sees a read behind it):
    malformed for all three, and taken by all three only when nothing is missing."""
    batch, streams = sc.one_pair_case()
    ints, dbls = len(streams.ints), len(streams.dbls)
    assert ints == 34 and dbls == 8
    lines = [line.split() for line in run(program, "cuts", sc.write_case(str(tmp_path / "pair.bin"), batch, streams))]
    assert [(w[0], int(w[1])) for w in lines] == [("i", n) for n in range(ints + 1)] + [("d", n) for n in range(dbls + 1)]
    for kind, n, sam, summary, refs in lines:
        whole = int(n) == (ints if kind == "i" else dbls)
        assert sam == summary == refs == ("1" if whole else "0"), (kind, n)
