"""GPU tier: the pairs of tests/pair_geometry.py against the oracle bit for bit, in every launch shape that runs other pairing code - the lane-per-read
passes with and without the pair's second lane and the handed-over regions, full waves, and the wave-per-read form, which has its own copy of the pairing
code and hands overlapping mates over to the lane passes - and the batch that must fail: queries for which the reference would have thrown
(tests/test_pair_geometry.py shows on the CPU that the oracle throws for each of them).

How a failed call names its query (xm_kernel_common.h, xm_capi.hip): every lane that ends a read with an error status takes the minimum of the pass's
errQuery and its query index, and the host throws after the first pass, or wave tier, that left one.  So the call names the lowest failing query of the first
failing pass: with throwers of one kind, which fail in the same pass, the lowest of them; with throwers of different kinds, one of them.

A call that fails leaves nothing behind (include/xmapper_hip.h): nothing is remembered, no streams of a "last call" exist for xm_sam_format_last and
xm_pileup_add_last, and a stream of batches leaves no staged batch."""
import os
import re
import subprocess
import sys
import tempfile
import threading
import numpy as np
import pytest

import oracle_lib as o
import pair_geometry as pg
from helpers import streams_equal, first_difference
from memo_helpers import expected_copies
from mapper_amd import api, hostio, pileup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = api.AlignmentParameters()
WOULD_HAVE_THROWN = "Failed to align query %d: the reference implementation would have thrown here"
SHAPES = {"default": {}, "one_lane_per_pair": {"XM_PAIR_LANES": "0"}, "no_handover": {"XM_HANDOVER": "0"}, "full_waves": {"XM_FULL_WAVES": "1", "XM_FULL_LPW": "32"},
          "wave_form": {"XM_WAVE": "1"}}
N_ORDINARY = 2000


class Work:
    pass


@pytest.fixture(scope="module")
def work():
    """The reference, its oracle and its database; per class the groups without the queries the oracle throws for, with the oracle's streams; 2 000 ordinary
    queries with the oracle's streams; one thrower of each kind.  Computed once."""
    w = Work()
    w.contigs, _ = pg.reference()
    w.oracle = o.OracleReference(w.contigs)
    w.db = api.ReferenceDatabase(w.contigs)
    w.classes = {}
    for name, make in pg.CLASSES.items():
        w.classes[name] = []
        for g in make():
            keep, _ = pg.split_throwers(w.oracle, g)
            w.classes[name].append((keep, pg.batch(keep), w.oracle.align(pg.batch(keep), o.make_params(keep.params))))   # (one thread: the counters are per worker)
    w.ordinary = pg.ordinary_queries(N_ORDINARY)
    w.want_ordinary = w.oracle.align(o.QueryBatch(w.ordinary), o.make_params(), threads=os.cpu_count())
    w.throwers = {kind: q for kind, (q, _) in pg.one_of_each_kind().items()}
    yield w
    w.db.close()


def gpu_align(db, batch, params=None):
    r = db.align_arrays(batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes, batch.expected_inner, batch.deviation, params or PARAMS)
    return o.Streams(r.ints, r.dbls, r.int_off, r.dbl_off, r.counters), r


def counters_match(dev, oracle):
    """Device counters against the oracle's (tests/test_gpu_wave.py): reads, probes, fetches, positions, candidates extended, PathAligner calls and nodes, quick accepts."""
    d, w = [int(x) for x in dev[:8]], [int(x) for x in oracle[:9]]
    return d == [w[0], w[1] + w[2], w[2], w[3], w[5], w[6], w[7], w[8]], (d, w)


def within(seconds, call):
    """call() on a thread of its own: its value, or its exception; a call that has not returned after `seconds` fails the test instead of holding the suite."""
    box = {}

    def run():
        try:
            box["value"] = call()
        except BaseException as e:  # noqa: BLE001  (raised again below)
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "the call has not returned after %d s" % seconds
    if "error" in box:
        raise box["error"]
    return box["value"]


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------- the classes against the oracle

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(pg.CLASSES))
def test_class_equals_the_oracle(name, shape, work, monkeypatch):
    set_env(monkeypatch, SHAPES[shape])
    for keep, batch, want in work.classes[name]:
        got, _ = gpu_align(work.db, batch, api.AlignmentParameters(**keep.params))
        assert streams_equal(got, want), first_difference(got, want, batch.nq)
        ok, detail = counters_match(got.counters, want.counters)
        assert ok, detail


# ---------------------------------------------------------------- the batch that must fail

def mixed(work, placed):
    return o.QueryBatch(pg.with_throwers(work.ordinary, placed))


def fails_naming(db, batch, q, seconds=120):
    with pytest.raises(RuntimeError, match=re.escape(WOULD_HAVE_THROWN % q)):
        within(seconds, lambda: gpu_align(db, batch))


def aligns_ordinary(db, work):
    got, r = within(120, lambda: gpu_align(db, o.QueryBatch(work.ordinary)))
    assert streams_equal(got, work.want_ordinary), first_difference(got, work.want_ordinary, N_ORDINARY)
    return r


@pytest.mark.parametrize("shape", ["default", "wave_form", "full_waves"])
@pytest.mark.parametrize("kind", pg.THROWER_KINDS)
def test_one_thrower_fails_the_batch(kind, shape, work, monkeypatch):
    """One thrower in the middle of 2 000 ordinary queries: the call names it, and the same context then aligns the batch without it as the oracle does.
    Under XM_FULL_WAVES=1 the thrower shares its wave with live reads; under XM_WAVE=1 the wave-per-read kernels meet it first."""
    set_env(monkeypatch, SHAPES[shape])
    fails_naming(work.db, mixed(work, [(1000, work.throwers[kind])]), 1000)
    aligns_ordinary(work.db, work)


@pytest.mark.parametrize("shape", ["default", "wave_form"])
def test_throwers_of_one_kind_name_the_lowest(shape, work, monkeypatch):
    set_env(monkeypatch, SHAPES[shape])
    for kind in pg.THROWER_KINDS:
        a, b, c = [q for k, q, _ in pg.throwers() if k.startswith(kind)][:3]
        fails_naming(work.db, mixed(work, [(1500, a), (300, b), (900, c)]), 300)
    aligns_ordinary(work.db, work)


@pytest.mark.parametrize("shape", ["default", "wave_form", "full_waves"])
def test_two_throwers_of_different_kinds_name_one_of_them(shape, work, monkeypatch):
    set_env(monkeypatch, SHAPES[shape])
    kinds = list(pg.THROWER_KINDS)
    for first, second in ((kinds[0], kinds[1]), (kinds[1], kinds[0]), (kinds[2], kinds[0])):
        with pytest.raises(RuntimeError, match="the reference implementation would have thrown here") as err:
            within(120, lambda: gpu_align(work.db, mixed(work, [(400, work.throwers[first]), (1200, work.throwers[second])])))
        assert int(re.search(r"Failed to align query (\d+)", str(err.value)).group(1)) in (400, 1200)
    aligns_ordinary(work.db, work)


def test_collapsed_throwers_name_their_representative(work):
    """Three byte-identical contained pairs at 900, 100 and 1700 are one group: the call names the lowest index (xm_context_set_collapse)."""
    c = work.db.new_context()
    try:
        c.set_collapse(True)
        q = work.throwers["contained"]
        fails_naming(c, mixed(work, [(900, q), (100, q), (1700, q)]), 100)
        r = aligns_ordinary(c, work)
        assert r.copies == expected_copies(o.QueryBatch(work.ordinary))
    finally:
        c.close()


def check_memory_after_failure(work, ctx, entries):
    """`ctx` remembers (entries() -> the records held): a failed call remembers nothing, the next good batch is served nothing of it, its repeat everything."""
    first = o.QueryBatch(work.ordinary[:300])
    gpu_align(ctx, first)
    before = entries()
    assert before > 0
    rest = work.ordinary[300:1100]
    fails_naming(ctx, o.QueryBatch(pg.with_throwers(rest, [(400, work.throwers["contained"])])), 400)
    assert entries() == before
    good = o.QueryBatch(rest)
    want = compose_batch_streams(work, range(300, 1100))
    got, r = gpu_align(ctx, good)
    assert r.extra[6] == 0 and r.remembered == 0
    assert streams_equal(got, want), first_difference(got, want, good.nq)
    assert entries() > before
    got, r = gpu_align(ctx, good)
    assert streams_equal(got, want) and r.remembered + r.copies == good.nq and r.counters[0] == 0


def compose_batch_streams(work, idx):
    """The oracle's streams of the ordinary queries idx, cut from its run over all of them."""
    idx = np.asarray(list(idx), np.int64)
    w = work.want_ordinary
    ints = np.concatenate([w.ints[w.int_off[q]:w.int_off[q + 1]] for q in idx])
    dbls = np.concatenate([w.dbls[w.dbl_off[q]:w.dbl_off[q + 1]] for q in idx])
    io = np.concatenate([[0], np.cumsum(w.int_off[idx + 1] - w.int_off[idx])]).astype(np.int64)
    do = np.concatenate([[0], np.cumsum(w.dbl_off[idx + 1] - w.dbl_off[idx])]).astype(np.int64)
    return o.Streams(ints, dbls, io, do)


def test_a_failed_call_remembers_nothing(work):
    c = work.db.new_context()
    try:
        c.set_memo(64 << 20)
        check_memory_after_failure(work, c, lambda: c.memo_info()["entries"])
    finally:
        c.close()


def test_a_failed_call_leaves_a_shared_memory_alone(work):
    c = work.db.new_context()
    memory = api.QueryMemory(work.db, 64 << 20)
    try:
        c.attach_memory(memory)
        check_memory_after_failure(work, c, lambda: memory.info()["entries"])
    finally:
        c.close()
        memory.close()


def arrays(batch):
    return batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes, batch.expected_inner, batch.deviation


def test_stream_with_a_thrower_in_its_second_batch(work):
    """align_stream: the first batch's result arrives, the generator raises at the second, and the context is as good as new: it aligns, and no batch is
    left staged (the third was being staged while the second ran)."""
    c = work.db.new_context()
    try:
        thirds = [work.ordinary[0:300], pg.with_throwers(work.ordinary[300:600], [(150, work.throwers["negative deviation"])]), work.ordinary[600:900]]
        stream = c.align_stream((arrays(o.QueryBatch(t)) for t in thirds), PARAMS)
        r = within(120, lambda: next(stream))
        want = compose_batch_streams(work, range(0, 300))
        assert streams_equal(r, want), first_difference(r, want, 300)
        with pytest.raises(RuntimeError, match=re.escape(WOULD_HAVE_THROWN % 150)):
            within(120, lambda: next(stream))
        with pytest.raises(StopIteration):
            next(stream)
        with pytest.raises(RuntimeError, match="no staged batch"):
            c.commit_staged()
        aligns_ordinary(c, work)
    finally:
        c.close()


def letters(codes):
    return api.decode(codes).encode()


def fastq_of(reads, name):
    return b"".join(b"@" + (name % i).encode() + b"\n" + letters(r) + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))


def test_last_streams_after_a_failed_call(work, tmp_path):
    """The same resident batch aligned twice.  Its spacing is (1000, -50): with MaxErrorRate 0.03 the window reaches (int)(300 * 0.03 * -50 + 1000) + 150 = 700
    bases and the exact pairs align; with the default rate it reaches -350, and the reference would have thrown for query 0.  After the failed call xm_sam_format_last and xm_pileup_add_last refuse - on a batch that was
    aligned before as on a freshly uploaded one - and the next successful call brings them back: the text is the host formatter's, byte for byte."""
    pairs = [m for m, _, _ in work.ordinary[:400] if len(m) == 2]
    open(tmp_path / "p1.fq", "wb").write(fastq_of([p[0] for p in pairs], "pair%d/1"))
    open(tmp_path / "p2.fq", "wb").write(fastq_of([p[1] for p in pairs], "pair%d/2"))
    (batch,) = hostio.read_batches(str(tmp_path / "p1.fq"), str(tmp_path / "p2.fq"), 1_000_000, expected_inner=1000.0, deviation=-50.0)
    names = [n for n, _ in work.contigs]
    refused = "the batch of the last align call is no longer resident"
    exact = api.AlignmentParameters(MaxErrorRate=0.03)
    c = work.db.new_context()
    piled = pileup.MatchDatabase(c)
    try:
        c.set_sam_contigs(names)
        c.upload_arrays(*batch.arrays())
        good = c.align_resident(exact)
        text = c.format_sam_last(batch)
        with tempfile.TemporaryFile("w+b") as f:
            hostio.Writer(names, f, None, threads=2).write(batch, good)
            f.seek(0)
            want = f.read()
        assert bytes(text) == want and want.count(b"\n") >= len(pairs)
        text.close()
        n = piled.add_last()
        assert n >= 0
        with pytest.raises(RuntimeError, match=re.escape(WOULD_HAVE_THROWN % 0)):
            c.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match=refused):
            c.format_sam_last(batch)
        with pytest.raises(RuntimeError, match=refused):
            piled.add_last()
        again = c.align_resident(exact)
        assert streams_equal(again, good)
        text = c.format_sam_last(batch)
        assert bytes(text) == want
        text.close()
        depth = piled._sum(0)[0].copy()
        piled.add_last()
        assert np.array_equal(piled._sum(0)[0], 2 * depth)   # (the refused call added nothing)
        # a freshly uploaded batch whose first call fails
        c.upload_arrays(*batch.arrays())
        with pytest.raises(RuntimeError, match=re.escape(WOULD_HAVE_THROWN % 0)):
            c.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match=refused):
            c.format_sam_last(batch)
        with pytest.raises(RuntimeError, match=refused):
            piled.add_last()
    finally:
        batch.close()
        piled.close()
        c.close()


def test_a_sibling_context_is_not_disturbed(work):
    a, b = work.db.new_context(), work.db.new_context()
    try:
        aligns_ordinary(b, work)
        fails_naming(a, mixed(work, [(1000, work.throwers["contained"])]), 1000)
        aligns_ordinary(b, work)
        aligns_ordinary(a, work)
    finally:
        a.close()
        b.close()


def test_command_line_fails_with_the_librarys_message(work, tmp_path):
    """A paired FASTQ file with one contained pair through `python -m mapper_amd`, as a child process under a time limit: non-zero exit, the library's message
    on stderr, no hang."""
    pairs = [m for m, _, _ in work.ordinary[:60] if len(m) == 2]
    pairs.insert(20, work.throwers["contained"][0])
    open(tmp_path / "p1.fq", "wb").write(fastq_of([p[0] for p in pairs], "pair%d/1"))
    open(tmp_path / "p2.fq", "wb").write(fastq_of([p[1] for p in pairs], "pair%d/2"))
    open(tmp_path / "ref.fa", "wb").write(b"".join(b">" + n.encode() + b"\n" + letters(c) + b"\n" for n, c in work.contigs))
    argv = [sys.executable, "-m", "mapper_amd", "--reference", str(tmp_path / "ref.fa"), "--paired-queries", str(tmp_path / "p1.fq"), str(tmp_path / "p2.fq"), "--spacing", "100", "50",
            "--out-sam", str(tmp_path / "out.sam")]
    out = subprocess.run(argv, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0, out.stdout + out.stderr
    assert WOULD_HAVE_THROWN % 20 in out.stderr, out.stderr
