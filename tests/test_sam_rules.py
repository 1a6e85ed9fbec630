"""SAM records as text, without a GPU: the rules the device formatter applies (mapper_amd/csrc/xm_sam_rules.h, plain C++ that the kernels of xm_sam.h call) run
by tests/sam_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the runtime), against
the host formatter (hostio.Writer, hostio.java_double), which defines the output; and the command line's --format-on-gpu."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sam_cases as sc
from mapper_amd import cli, hostio

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "sam_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/sam_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("sam_rules") / "sam_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + list(args), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def python_formatter_values():
    """The values of tests/test_hostio.py test_java_double_matches_the_python_formatter."""
    rng = np.random.default_rng(8)
    vals = [0.0, 1.0, 0.1, 0.5, 10.0, 1e7, 9999999.999, 1e-3, 0.00099999, 1e-5, 1.5e300, 123456.789, 0.30000000000000004, 1 / 3, 1e22, 5e-324, -2.5, 84743373.69372326]
    vals += list(rng.random(2000) * rng.choice([1, 10, 100, 1e-3, 1e4, 1e6, 1e8], 2000)) + [x * 0.1 for x in range(1000)] + [x / 20 for x in range(2000)]
    vals += list(rng.integers(0, 2**63, 2000).astype(np.uint64).view(np.float64))
    return np.array(vals, np.float64)


def test_doubles_equal_to_chars_over_the_corpus(program, tmp_path):
    """Powers of two and ten with their neighbours, the subnormal and normal limits, the switch of notation, -0.0, NaN, the infinities, 1.2 M random bit
    patterns, 1.1 M penalty sums, and the values of the Python formatter's test: the program compares with std::to_chars and stops at the first difference."""
    path = str(tmp_path / "values.f64")
    python_formatter_values().tofile(path)
    out = run(program, "doubles", path).decode().split()
    assert out[0] == "ok" and int(out[1]) >= 2_000_000 and out[2] == "maxlen" and int(out[3]) <= 24, out


def test_doubles_equal_the_host_formatter(program, tmp_path):
    vals = np.concatenate([python_formatter_values(), [9999999.999999998, 1.0e7, 0.001, 9.999999999999999e-4, -0.0, 2.2250738585072014e-308, 1.7976931348623157e308, 5e-324,
                                                       float("inf"), float("-inf"), 0.6000000000000001, 12345678.0, 100.0]])
    path = str(tmp_path / "values.f64")
    vals.tofile(path)
    got = run(program, "strings", path).decode().split("\n")[:-1]
    assert len(got) == len(vals)
    for v, g in zip(vals, got):
        if v == v:
            assert g == hostio.java_double(v), v
    assert max(len(g) for g in got) <= 24


def format_case(program, tmp_path, batch, streams):
    """The program's text for the case, or ("malformed", query)."""
    out = run(program, "format", sc.write_case(str(tmp_path / "case.bin"), batch, streams))
    head, _, text = out.partition(b"\n")
    words = head.split()
    if words[0] == b"malformed":
        return ("malformed", int(words[1]))
    assert words[0] == b"ok" and int(words[1]) == len(text) and int(words[2]) == text.count(b"\n")
    return text


def test_records_of_every_shape_equal_the_host_formatter(program, tmp_path):
    batch, streams = sc.shapes_case()
    want = sc.expected(batch, streams)
    assert want.count(b"\n") == 40 and b"\t2147483648\t" in want and b"4S40M6S" in want and b"\t50M\t" in want and b"10M3I4D5M3D3I30M" in want
    assert format_case(program, tmp_path, batch, streams) == want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_records_equal_the_host_formatter(program, tmp_path, seed):
    batch, streams = sc.random_case(seed, 400)
    want = sc.expected(batch, streams)
    assert want.count(b"\n") > 400
    assert format_case(program, tmp_path, batch, streams) == want


def test_unaligned_queries_and_one_query_with_three_alignments(program, tmp_path):
    assert format_case(program, tmp_path, *sc.all_unaligned_case(70)) == b""
    batch, streams = sc.three_alignments_case()
    want = sc.expected(batch, streams)
    assert want.count(b"\n") == 3 and format_case(program, tmp_path, batch, streams) == want


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_a_malformed_slice_is_reported_with_its_lowest_query(program, tmp_path, name):
    batch, streams, query = sc.malformed_cases()[name]
    with pytest.raises(RuntimeError, match="malformed result streams"):  # (the host formatter refuses the same streams)
        sc.expected(batch, streams)
    assert format_case(program, tmp_path, batch, streams) == ("malformed", query)


def test_a_slice_cut_short_anywhere_is_malformed_and_nothing_behind_it_is_read(program, tmp_path):
    batch, streams = sc.one_pair_case()
    ints, dbls = len(streams.ints), len(streams.dbls)
    assert ints == 34 and dbls == 8
    out = run(program, "cut", sc.write_case(str(tmp_path / "pair.bin"), batch, streams))  # (every cut in a heap block of its own size: the sanitizer build sees a read behind it)
    assert out.split() == [b"cut", b"ok", b"%d" % ints, b"%d" % dbls], out


def test_cli_flag_and_what_it_excludes():
    base = ["--reference", "r.fa", "--out-sam", "o.sam", "--queries", "q.fq"]
    assert cli.parse_args(base + ["--format-on-gpu"])["format_on_gpu"] is True
    assert not cli.parse_args(base).get("format_on_gpu")
    both = cli.parse_args(base + ["--format-on-gpu", "--parse-on-gpu", "--format-threads", "4"])
    assert both["format_on_gpu"] is True and both["parse_on_gpu"] is True and both["format_threads"] == 4
    with pytest.raises(cli.UsageError, match="--per-object"):
        cli.parse_args(base + ["--format-on-gpu", "--per-object"])
    with pytest.raises(cli.UsageError, match="--out-mutations"):
        cli.parse_args(base + ["--format-on-gpu", "--out-mutations", "m.txt"])
    with pytest.raises(cli.UsageError, match="--out-refs-map-count"):
        cli.parse_args(base + ["--out-refs-map-count", "c.txt", "--format-on-gpu"])
    with pytest.raises(cli.UsageError, match="--format-threads"):
        cli.parse_args(base + ["--format-threads", "0"])
