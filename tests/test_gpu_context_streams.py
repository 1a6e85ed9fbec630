"""Contexts of one GPU side by side: every context aligns on a stream of its own, all of them stage their batches through ONE copy stream that the
shared device tables own (DeviceTables::copyStream), and the tables keep no stream of their own between uploads.  What can go wrong with that is an ordering
that used to be implicit (a copy or a fill of one context seen by another, a staged batch committed before its copy has landed, a copy stream that goes away
with the context that made it, tables that grow while another context's kernels read them): every test runs contexts at the same time on threads and
compares what they return, bit for bit, with what ONE context returns for the same batch aligned alone.

Shapes: 3 000 to 5 000 reads of 150 bp on a 200 kb reference - more than one block of every bookkeeping kernel, several passes per call (indel_prob 0.3 sends
reads to the gapped pass: counters[5], the PathAligner calls, is asserted > 0), a fraction of a second per call."""
import threading

import numpy as np
import pytest

from helpers import se_batch
from mapper_amd import api, synth

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
REF_LEN = 200_000
N_BATCHES = 4


def arrays_of(b):
    return (b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation)


def bits(r):
    """the four result streams of a BatchResult; penalties as their bits"""
    return (np.array(r.ints), np.array(r.dbls).view(np.int64), np.array(r.int_off), np.array(r.dbl_off))


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def run_threads(targets):
    """every target on a thread of its own; the first exception of any of them is raised here"""
    errors = []

    def guard(f):
        def g():
            try:
                f()
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        return g
    th = [threading.Thread(target=guard(f)) for f in targets]
    [t.start() for t in th]
    [t.join() for t in th]
    if errors:
        raise errors[0]


@pytest.fixture(scope="module")
def world():
    """The reference, four contexts' worth of batches (a seed per context and batch) and what one fresh context returns for each of them alone."""
    ref = synth.synthetic_reference(REF_LEN, seed=0xC0FFEE)
    batches = [[arrays_of(se_batch(synth.synthetic_single_end(ref, 3000, read_len=150, seed=7000 + 16 * c + k, indel_prob=0.3)[0])) for k in range(N_BATCHES)] for c in range(4)]
    alone = api.ReferenceDatabase([("r", ref)])
    want = []
    for per_context in batches:
        row = []
        for a in per_context:
            r = alone.align_arrays(*a, PARAMS)
            assert r.counters[5] > 0, "no read of the batch reached the gapped pass"
            row.append(bits(r))
        want.append(row)
    alone.close()
    return {"ref": ref, "batches": batches, "want": want}


def stream_all(ctx, batches, got, i):
    got[i] = [bits(r) for r in ctx.align_stream(iter(batches), PARAMS)]


@pytest.mark.parametrize("n_ctx", [3, 4])
def test_concurrent_streaming_equals_serial(world, n_ctx):
    db = api.ReferenceDatabase([("r", world["ref"])])
    ctx = [db] + [db.new_context() for _ in range(n_ctx - 1)]
    got = [None] * n_ctx
    run_threads([lambda i=i: stream_all(ctx[i], world["batches"][i], got, i) for i in range(n_ctx)])
    for i in range(n_ctx):
        assert len(got[i]) == N_BATCHES
        for k in range(N_BATCHES):
            assert same(got[i][k], world["want"][i][k]), "context %d of %d, batch %d differs from the batch aligned alone" % (i, n_ctx, k)
    for c in ctx[1:]:
        c.close()
    db.close()


def test_shared_copy_stream_outlives_the_context_that_created_it(world):
    """The database's first context stages first (the copy stream comes into being then) and is closed while two other contexts stream; they finish with the
    same results, and a context made afterwards streams too."""
    first = api.ReferenceDatabase([("r", world["ref"])])
    others = [first.new_context(), first.new_context()]
    got0 = [bits(r) for r in first.align_stream(iter(world["batches"][0][:1]), PARAMS)]
    assert same(got0[0], world["want"][0][0])
    under_way = [threading.Event(), threading.Event()]

    def feed(i):  # the context's batches; says when the second one has been asked for (the first is being aligned then)
        for k, a in enumerate(world["batches"][i + 1]):
            if k == 1:
                under_way[i].set()
            yield a
    got = [None, None]

    def stream(i):
        try:
            got[i] = [bits(r) for r in others[i].align_stream(feed(i), PARAMS)]
        finally:
            under_way[i].set()

    def close_first():
        [e.wait() for e in under_way]
        first.close()
    run_threads([lambda: stream(0), lambda: stream(1), close_first])
    for i in range(2):
        assert len(got[i]) == N_BATCHES
        for k in range(N_BATCHES):
            assert same(got[i][k], world["want"][i + 1][k]), "context %d, batch %d differs after the first context was closed" % (i + 1, k)
    late = others[0].new_context()
    got_late = [bits(r) for r in late.align_stream(iter(world["batches"][3]), PARAMS)]
    for k in range(N_BATCHES):
        assert same(got_late[k], world["want"][3][k]), "context made after the close, batch %d" % k
    late.close()
    for c in others:
        c.close()


def test_tables_grow_while_another_context_aligns(world):
    """max_query_length=150: a 260 bp batch makes its context hash further lengths and upload the tables again (ensureTablesFor -> upload, which creates and
    destroys its stream) while another context aligns 150 bp batches in a loop."""
    ref = world["ref"]
    short = world["batches"][0][0]
    long_ = arrays_of(se_batch(synth.synthetic_single_end(ref, 3000, read_len=260, seed=7777, indel_prob=0.3)[0]))
    alone = api.ReferenceDatabase([("r", ref)], max_query_length=150)
    want_short = bits(alone.align_arrays(*short, PARAMS))
    want_long = bits(alone.align_arrays(*long_, PARAMS))
    alone.close()
    assert same(want_short, world["want"][0][0])
    db = api.ReferenceDatabase([("r", ref)], max_query_length=150)
    other = db.new_context()
    started, grown = threading.Event(), threading.Event()
    got_short, got_long = [], []

    def loop():
        try:
            while True:
                last = grown.is_set()
                got_short.append(bits(db.align_arrays(*short, PARAMS)))
                started.set()
                if last:  # (one more call after the tables have grown)
                    return
        finally:
            started.set()

    def grow():
        try:
            started.wait()
            got_long.append(bits(other.align_arrays(*long_, PARAMS)))
        finally:
            grown.set()
    run_threads([loop, grow])
    assert other.info()["max_hashed_length"] >= 260
    assert len(got_long) == 1 and same(got_long[0], want_long)
    assert len(got_short) >= 2
    for k, g in enumerate(got_short):
        assert same(g, want_short), "150 bp batch, call %d of %d" % (k, len(got_short))
    other.close()
    db.close()


def test_resident_batches_of_three_contexts(world):
    """Three contexts, each with the same 5 000 reads resident, call align_resident from three threads, three rounds each."""
    ref = world["ref"]
    a = arrays_of(se_batch(synth.synthetic_single_end(ref, 5000, read_len=150, seed=8181, indel_prob=0.3)[0]))
    db = api.ReferenceDatabase([("r", ref)])
    r = db.align_arrays(*a, PARAMS)
    assert r.counters[5] > 0
    want = bits(r)
    ctx = [db, db.new_context(), db.new_context()]
    for c in ctx:
        c.upload_arrays(*a)
    got = [[] for _ in ctx]

    def rounds(i):
        for _ in range(3):
            got[i].append(bits(ctx[i].align_resident(PARAMS)))
    run_threads([lambda i=i: rounds(i) for i in range(len(ctx))])
    for i in range(len(ctx)):
        for k in range(3):
            assert same(got[i][k], want), "context %d, round %d" % (i, k)
    for c in ctx[1:]:
        c.close()
    db.close()
