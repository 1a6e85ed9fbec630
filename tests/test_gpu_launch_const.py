"""The launch block of the lane-per-read kernel (LaunchConst, mapper_amd/csrc/xm_defs.h): the index view and the alignment parameters of a launch live in one
block per context in HBM, written on the context's stream in front of every launch (PassBuffers::launchConst, xm_capi.hip), and the lanes read them through it.
What can go wrong is a launch that reads a block that is not its own: the last call's parameters, another context's, the view from before the tables grew, the
confidence table from before it moved.  Every case below changes one of those between launches and compares every call bit for bit with the oracle.

Shapes: 130 single reads of 150 bases (three waves, the last not full), 70 pairs, 40 reads of 40 lengths, 150 reads of 260 bases - the smallest at which
the passes in question run; each assert says which pass it relies on.  The oracle aligns every (batch, parameters) once per module."""
import threading

import numpy as np
import pytest

import oracle_lib as o
from helpers import streams_equal, first_difference, se_batch, ragged_se_batch, pe_batch, sprinkle_ambiguity, alignments_per_query
from mapper_amd import api, synth

pytestmark = pytest.mark.gpu

REF_LEN = 60_000
P1 = {}                                                        # Mapper's defaults
P2 = {"MutationPenalty": 1.5, "Max_PenaltySpan": 2.0}          # other penalties: other confidence keys, other candidate sets, other totals
P3 = {"MutationPenalty": 0.75, "Max_PenaltySpan": 1.0}


def api_params(d):
    return api.AlignmentParameters(**d)


def with_deletion(ref, start, length, at, n):
    """`length` bases of ref from `start` with n bases deleted in front of index `at`"""
    t = ref[start:start + length + n]
    return np.concatenate([t[:at], t[at + n:]])[:length].copy()


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.ref = synth.synthetic_reference(REF_LEN, seed=0xEC011)
    rng = np.random.default_rng(0x1C0457)
    plain = synth.synthetic_single_end(w.ref, 100, seed=0x5EED0011)[0]
    # reads with a 3-base deletion away from their ends: their straight alignment is too expensive, so the gapped pass aligns them
    gapped = np.stack([with_deletion(w.ref, int(rng.integers(0, REF_LEN - 200)), 150, int(rng.integers(50, 100)), 3) for _ in range(20)])
    amb = sprinkle_ambiguity(synth.synthetic_single_end(w.ref, 10, seed=0x5EED0012)[0], seed=5)
    amb[0, 20] = 15  # (at least one read with an ambiguity code whatever the sprinkling drew)
    w.singles = se_batch(np.concatenate([plain, gapped, amb]))
    assert w.singles.nq == 130
    m1, m2 = synth.synthetic_paired_end(w.ref, 70, seed=0x5EED0013)[:2]
    m1 = m1.copy()
    m1[::10] = sprinkle_ambiguity(m1[::10], seed=6)
    w.pairs = pe_batch(m1, m2)
    # 40 reads of 40 lengths: with an empty confidence table every length is a key of its own, so the first pass leaves reads waiting and the table
    # grows (and moves) before they run again
    # (one substitution each, in the middle: a read of penalty 0 is accepted before the table is asked)
    ragged = [w.ref[s:s + L].copy() for s, L in zip(rng.integers(0, REF_LEN - 200, 40), range(100, 140))]
    for r in ragged:
        r[len(r) // 2] = {1: 2, 2: 4, 4: 8, 8: 1}[int(r[len(r) // 2])]
    w.ragged = ragged_se_batch(ragged)
    # one read with many ambiguous bases among plain ones: its pyramid outgrows the capacities of scale 1 and it runs again at scale 4
    rerun = synth.synthetic_single_end(w.ref, 12, seed=0x5EED0014)[0].copy()
    rerun[3, rng.random(150) < 0.5] = 15
    w.scale = se_batch(rerun)
    w.long = se_batch(synth.synthetic_single_end(w.ref, 150, read_len=260, seed=0x5EED0015)[0])
    w.oracle = o.OracleReference([("r", w.ref)], mode="mapper")
    w.want = {}
    return w


def want(w, name, params):
    key = (name, tuple(sorted(params.items())))
    if key not in w.want:
        w.want[key] = w.oracle.align(getattr(w, name), o.make_params(params), threads=8)
    return w.want[key]


def check(got, wanted, b, what):
    """streams and offsets bit for bit; counters[0:8] against the oracle's as tests/test_gpu_parity.py maps them, [8] the alignments in the oracle's streams,
    [10] the bytes of the reads as 4-bit codes.  -> counters[0:11] (refWindowBytes, [9], has no oracle counterpart: the callers compare it between calls that must agree)"""
    s = o.Streams(got.ints, got.dbls, got.int_off, got.dbl_off, got.counters)
    assert streams_equal(s, wanted), (what, first_difference(s, wanted, b.nq))
    assert np.array_equal(got.int_off, wanted.int_off) and np.array_equal(got.dbl_off, wanted.dbl_off), what
    oc = [int(x) for x in wanted.counters[:9]]
    c = [int(x) for x in got.counters[:11]]
    assert c[:8] == [oc[0], oc[1] + oc[2], oc[2], oc[3], oc[5], oc[6], oc[7], oc[8]], what
    assert c[8] == int(np.sum(alignments_per_query(wanted))), what
    assert c[10] == int(((b.mate_length.astype(np.int64) + 1) // 2).sum()), what
    return c


def upload(ctx, b):
    ctx.upload_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation)


@pytest.mark.parametrize("name", ["singles", "pairs"])
def test_parameters_change_from_call_to_call(world, name):
    """One resident batch, one context, three calls: Mapper's defaults, other penalties, the defaults again.  A launch that read the block of the call before it
    would give that call's alignments.  The singles hold reads with a deletion, so every call has a gapped pass (counters[5]: PathAligner calls)."""
    b = getattr(world, name)
    db = api.ReferenceDatabase([("r", world.ref)], mode="mapper")
    upload(db, b)
    seen = []
    for params in (P1, P2, P1):
        got = db.align_resident(api_params(params))
        seen.append(check(got, want(world, name, params), b, (name, params)))
        if name == "singles":
            assert seen[-1][5] > 0, "no PathAligner call: the gapped pass did not run"
    assert seen[0] == seen[2]
    w1, w2 = want(world, name, P1), want(world, name, P2)
    assert not (np.array_equal(w1.dbls, w2.dbls) and np.array_equal(w1.ints, w2.ints)), "the two parameter sets give the same streams: the case proves nothing"
    db.close()


def test_two_contexts_with_their_own_parameters(world):
    """Two contexts of one index align at the same time from two threads, each with its own parameters, three rounds: the block is the context's, not the GPU's."""
    db = api.ReferenceDatabase([("r", world.ref)], mode="mapper")
    ctxs = [db, db.new_context()]
    params = [P2, P3]
    for c in ctxs:
        upload(c, world.singles)
    got = [[None] * 3, [None] * 3]
    errors = []
    start = threading.Barrier(2)

    def work(i):
        try:
            for r in range(3):
                start.wait(timeout=60)
                got[i][r] = ctxs[i].align_resident(api_params(params[i]))
        except Exception as e:  # (reported by the main thread)
            errors.append(e)
            start.abort()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        seen = [check(got[i][r], want(world, "singles", params[i]), world.singles, ("context", i, "round", r)) for r in range(3)]
        assert seen[0] == seen[1] == seen[2]
    ctxs[1].close()
    db.close()


def test_view_after_the_tables_grew(world):
    """An index built for 150 bases aligns 260-base reads (xm_index_ensure_length grows the tables: other table pointers, another maxHashedLength in the view),
    then the 150-base batch again."""
    db = api.ReferenceDatabase([("r", world.ref)], mode="mapper", max_query_length=150)
    assert db.info()["max_hashed_length"] < 260
    first = check(db.align_arrays(*arrays(world.singles), api_params(P1)), want(world, "singles", P1), world.singles, "150 bases, before")
    check(db.align_arrays(*arrays(world.long), api_params(P1)), want(world, "long", P1), world.long, "260 bases")
    assert db.info()["max_hashed_length"] >= 260
    again = check(db.align_arrays(*arrays(world.singles), api_params(P1)), want(world, "singles", P1), world.singles, "150 bases, after")
    assert first == again
    db.close()


def arrays(b):
    return b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation


def test_view_changes_between_the_passes_of_a_call(world, monkeypatch):
    """XM_CONF_SEED=0: the confidence table starts empty, so reads of 40 lengths leave 40 keys in the miss list, the host evaluates them, the table grows and
    moves, and the rerun's launch must read the new view (counters[11]: reads run again; counters[7]: they were accepted through the table in the end)."""
    monkeypatch.setenv("XM_CONF_SEED", "0")
    db = api.ReferenceDatabase([("r", world.ref)], mode="mapper")
    got = db.align_arrays(*arrays(world.ragged), api_params(P1))
    check(got, want(world, "ragged", P1), world.ragged, "confidence rerun")
    assert int(got.counters[11]) > 0, "no read ran again: the confidence table was not empty"
    assert int(got.counters[7]) > 0, "no read was accepted through the confidence table"
    got = db.align_arrays(*arrays(world.ragged), api_params(P2))   # (other penalties: other keys, the table grows again)
    check(got, want(world, "ragged", P2), world.ragged, "confidence rerun, other parameters")
    db.close()


def test_scale_rerun_between_the_passes_of_a_call(world):
    """A read whose ambiguity outgrows the capacities of scale 1 runs again at scale 4 in a launch of its own (counters[11]), between two plain calls."""
    db = api.ReferenceDatabase([("r", world.ref)], mode="mapper")
    got = db.align_arrays(*arrays(world.scale), api_params(P1))
    check(got, want(world, "scale", P1), world.scale, "scale rerun")
    assert int(got.counters[11]) > 0, "no read ran again at a larger scale"
    check(db.align_arrays(*arrays(world.singles), api_params(P2)), want(world, "singles", P2), world.singles, "after the scale rerun")
    db.close()
