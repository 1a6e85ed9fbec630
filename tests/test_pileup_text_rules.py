"""The text of the pile-up's insertion events, without a GPU: the rules the kernels of xm_pileup_text.h and xm_pileup_add_last apply
(mapper_amd/csrc/xm_pileup_text_rules.h, plain C++) run by tests/pileup_text_main.cpp, a stand-alone program built here with g++ (with
-fsanitize=address,undefined where the host compiler has the runtime), against api.decode / api.reverse_complement, which define the text; the host's
ordering of a call's events with their text; the paging; and the command line's decision which jobs still need objects."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pileup_text_cases as tc
from mapper_amd import cli

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "pileup_text_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/pileup_text_main.cpp")
    out = str(tmp_path_factory.mktemp("pileup_text") / "pileup_text_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def files(tmp_path, **arrays):
    paths = {}
    for name, a in arrays.items():
        paths[name] = str(tmp_path / (name + ".bin"))
        np.ascontiguousarray(a).tofile(paths[name])
    return paths


def program_text(program, tmp_path, mate_offset, mate_length, codes, events, query_base=0):
    p = files(tmp_path, off=mate_offset.astype(np.int64), len=mate_length.astype(np.int32), codes=codes.astype(np.uint8), events=np.asarray(events, np.int64))
    out = run(program, "text", p["off"], p["len"], p["codes"], p["events"], query_base)
    n = len(events)
    return np.frombuffer(out[:8 * (n + 1)], np.int64), out[8 * (n + 1):]


def test_the_rule_equals_decode_of_the_oriented_slice(program, tmp_path):
    """Random mates with all 16 codes, both mates and orientations, startA of 0 and of readLen - length, deletions in between, and clipped events."""
    mate_offset, mate_length, codes = tc.synthetic_mates(40, seed=1)
    events = tc.random_events(3000, mate_length, seed=2, query_base=500)
    ins = events[events[:, 2] == 1]
    read_len = mate_length[2 * (ins[:, 4] - 500) + (ins[:, 5] & 1)]
    # the shapes are there: both orientations and mates, the two edge starts, the three clipped forms, every code inside an insertion
    assert set(ins[:, 5]) == {0, 1, 2, 3} and (events[:, 2] == 2).sum() > 500
    whole = (ins[:, 3] > 0) & (ins[:, 6] + ins[:, 3] <= read_len)
    assert (whole & (ins[:, 6] == 0)).any() and (whole & (ins[:, 6] == read_len - ins[:, 3]) & (ins[:, 6] > 0)).any()
    assert ((ins[:, 6] < read_len) & (ins[:, 6] + ins[:, 3] > read_len)).any() and (ins[:, 6] == read_len).any() and (ins[:, 6] > read_len).any() and (ins[:, 3] == 0).any()
    want_off, want = tc.rule_text(mate_offset, mate_length, codes, events, 500)
    assert set(want) == set(b"?ACMGRSVTWYHKDBN")
    off, text = program_text(program, tmp_path, mate_offset, mate_length, codes, events, 500)
    assert np.array_equal(off, want_off) and text == want


def test_every_code_in_both_orientations(program, tmp_path):
    codes = np.arange(16, dtype=np.uint8)
    events = [tc.event(0, 0, 0, 0, 16), tc.event(0, 0, 1, 0, 16), tc.event(0, 0, 1, 5, 3), tc.event(0, 0, 0, 13, 3)]
    off, text = program_text(program, tmp_path, np.array([0, 16]), np.array([16, 0]), codes, events)
    # (the reverse complement of ?ACMGRSVTWYHKDBN: N stays N, B <-> V, D <-> H, K <-> M, ...)
    assert text == b"?ACMGRSVTWYHKDBN" + b"NVHMDRWABSYCKGT?" + b"RWA" + b"DBN" and list(off) == [0, 16, 32, 35, 38]


def test_events_that_keep_nothing(program, tmp_path):
    """A deletion, length 0, a negative length, startA at and behind the mate's end and in front of the mate, a query of another batch, the empty mate 2 of a
    single read: no byte; an insertion that runs over the mate's end keeps what is inside."""
    codes = np.array([1, 2, 4, 8, 15], np.uint8)
    events = [tc.event(0, 0, 0, 1, 3, kind=2), tc.event(0, 0, 0, 1, 0), tc.event(0, 0, 0, 1, -4), tc.event(0, 0, 0, 5, 2), tc.event(0, 0, 1, 9, 2), tc.event(0, 0, 0, -1, 3),
              tc.event(1, 0, 0, 0, 2), tc.event(-1, 0, 0, 0, 2), tc.event(0, 1, 0, 0, 2), tc.event(0, 0, 0, 3, 9), tc.event(0, 0, 1, 3, 2**40)]
    off, text = program_text(program, tmp_path, np.array([0, 5]), np.array([5, 0]), codes, events)
    assert list(np.diff(off)) == [0] * 9 + [2, 2] and text == b"TN" + b"GT"
    want_off, want = tc.rule_text(np.array([0, 5]), np.array([5, 0]), codes, events)
    assert np.array_equal(off, want_off) and text == want
    off, text = program_text(program, tmp_path, np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((0, 8), np.int64))
    assert list(off) == [0] and text == b""


def test_text_follows_its_event_through_the_ordering_of_a_call(program, tmp_path):
    """Two calls into one pile-up: each call's events come out in (query, contig, position, flags, startA) order, call after call, and every event still
    owns the bytes it came with."""
    rng = np.random.default_rng(5)
    n, split = 700, 450
    events = np.zeros((n, 8), np.int64)
    events[:, 4] = np.where(np.arange(n) < split, rng.integers(0, 40, n), rng.integers(40, 60, n))   # (ordinals run on across the calls)
    events[:, 0] = rng.integers(0, 3, n)
    events[:, 1] = rng.integers(0, 50, n)
    events[:, 5] = rng.integers(0, 8, n)
    events[:, 6] = rng.integers(0, 4, n)
    events[:, 2] = rng.integers(1, 3, n)
    events[:, 3] = rng.integers(1, 30, n)
    events[:, 7] = np.arange(n)   # (a tag: which event this was)
    lengths = np.where(events[:, 2] == 1, events[:, 3], 0)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    text = rng.integers(65, 91, int(off[-1])).astype(np.uint8)
    p = files(tmp_path, events=events, off=off, text=text)
    out = run(program, "append", p["events"], p["off"], p["text"], split)
    got_events = np.frombuffer(out[:64 * n], np.int64).reshape(n, 8)
    got_off = np.frombuffer(out[64 * n:64 * n + 8 * (n + 1)], np.int64)
    got_text = out[64 * n + 8 * (n + 1):]
    order = sorted(range(split), key=lambda i: tc.event_order(events[i]) + (i,)) + sorted(range(split, n), key=lambda i: tc.event_order(events[i]) + (i,))
    assert np.array_equal(got_events, events[order]) and len(set(tuple(e) for e in events[:, [4, 0, 1, 5, 6]])) < n   # (ties are there, and keep their order)
    assert got_off[0] == 0 and got_off[-1] == len(text) == len(got_text) and np.all(np.diff(got_off) == lengths[order])
    for k, i in enumerate(order):
        assert got_text[got_off[k]:got_off[k + 1]] == text[off[i]:off[i + 1]].tobytes(), (k, i)
    assert order != list(range(n))


def test_paging_serves_as_many_events_as_fit_and_at_least_one(program, tmp_path):
    off = np.array([0, 3, 3, 10, 10, 10, 1010, 1011], np.int64)   # seven events: 3, 0, 7, 0, 0, 1000 and 1 bytes
    p = files(tmp_path, off=off)
    page = lambda first, n, cap: int(run(program, "page", p["off"], first, n, cap))  # noqa: E731
    assert page(0, 7, 1 << 20) == 7 and page(0, 7, 1011) == 7 and page(0, 7, 1010) == 6 and page(0, 7, 10) == 5 and page(0, 7, 9) == 2 and page(0, 7, 3) == 2
    assert page(0, 7, 2) == -1 and page(0, 7, 0) == -1          # the first event alone does not fit
    assert page(1, 6, 0) == 1 and page(3, 4, 0) == 2            # events without text fit into nothing
    assert page(5, 2, 999) == -1 and page(5, 2, 1000) == 1 and page(5, 2, 1001) == 2 and page(5, 1, 5000) == 1
    assert page(7, 4, 100) == 0 and page(0, 0, 100) == 0 and page(8, 1, 100) == -1 and page(-1, 1, 100) == -1 and page(0, 1, -1) == -1
    assert page(2, 100, 2**63 - 1) == 5


def test_which_jobs_need_objects():
    base = ["--reference", "r.fa", "--queries", "q.fq"]
    needs = lambda *flags: cli.needs_objects(cli.parse_args(base + list(flags)))  # noqa: E731
    assert not needs("--out-sam", "o.sam")
    assert not needs("--out-mutations", "m.txt") and not needs("--out-mutations", "m.txt", "--out-sam", "o.sam", "--out-unaligned", "u.fq")
    assert not needs("--out-mutations", "m.txt", "--parse-on-gpu") and not needs("--out-mutations", "m.txt", "--devices", "0,0")
    assert needs("--out-mutations", "m.txt", "--per-object") and needs("--per-object", "--out-sam", "o.sam")
    assert needs("--out-refs-map-count", "c.txt") and needs("--out-mutations", "m.txt", "--out-refs-map-count", "c.txt")
    with pytest.raises(cli.UsageError, match="--out-mutations"):   # (stays refused)
        cli.parse_args(base + ["--format-on-gpu", "--out-mutations", "m.txt"])
    with pytest.raises(cli.UsageError, match="--per-object"):
        cli.parse_args(base + ["--parse-on-gpu", "--per-object", "--out-mutations", "m.txt"])
