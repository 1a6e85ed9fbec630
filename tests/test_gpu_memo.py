"""GPU tier: queries a context has aligned are remembered across batches and repeats are served from HBM (xm_context_set_memo, api.ReferenceDatabase.set_memo;
the run-wide AlignmentCache of the reference's AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291).  The invariant: a query is only ever served from a
byte-identical query this context aligned earlier under bit-identical parameters - so the four streams never change, xm_result.extra[6] (BatchResult.remembered)
counts the representatives served, and the work counters count what was still aligned.  Expected counts come from the queries' keys (memo_helpers)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import streams_equal, first_difference
from memo_helpers import (PARAMS, align, arrays_of, batch_of, duplicated, expected_copies, expected_remembered, first_occurrences, key_of, keys_of, mixed_distinct, near_copies,
                          not_held, oracle_sample_equal, random_queries, sub_batch, unaligned_count)
from mapper_amd import api, multi, pileup, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMO = 64 << 20
MIN_MEMO = 64 << 10


@pytest.fixture(scope="module")
def ref():
    return synth.synthetic_reference(1_000_000, seed=0x3E3000)


@pytest.fixture(scope="module")
def db(ref):
    d = api.ReferenceDatabase([("syn", ref)])
    yield d
    d.close()


class Pair:
    """Batch A, then batch B: half of A's distinct queries, new queries, B's own duplicates, near-copies of A's queries; and what a plain context returns."""


@pytest.fixture(scope="module")
def ab(ref, db):
    rng = np.random.default_rng(0x3E31)
    distinct_a = mixed_distinct(ref, 1_000, 400, seed=0x3E32)
    half = [distinct_a[i] for i in rng.permutation(len(distinct_a))[:len(distinct_a) // 2]]
    near = near_copies(distinct_a, rng)
    queries_b = duplicated(half + mixed_distinct(ref, 500, 200, seed=0x3E34), seed=0x3E35) + near
    s = Pair()
    s.a = batch_of(duplicated(distinct_a, seed=0x3E33))
    s.b = batch_of([queries_b[i] for i in rng.permutation(len(queries_b))])
    assert 2_000 <= s.a.nq <= 4_000 and 2_000 <= s.b.nq <= 4_000
    plain = db.new_context()
    s.plain_a, s.plain_b = align(plain, s.a), align(plain, s.b)
    plain.close()
    s.keys_a, s.keys_b = keys_of(s.a), keys_of(s.b)
    s.remembered_b = expected_remembered(s.b, s.keys_a)
    assert s.remembered_b > 500 and not (keys_of(batch_of(near)) & s.keys_a)  # (the near-copies are none of A's)
    return s


def remembering(d, nbytes=MEMO):
    c = d.new_context()
    c.set_memo(nbytes)
    return c


def check_served(got, plain, b, held, d):
    """The assertions of a batch b on a context whose memory holds `held`: streams, counts, and the work of the queries that were still aligned."""
    assert streams_equal(got, plain), first_difference(got, plain, b.nq)
    assert got.remembered == expected_remembered(b, held) and got.copies == expected_copies(b)
    assert got.counters[0] == b.nq - got.remembered - got.copies
    rest = not_held(b, held)
    if rest:
        alone = d.new_context()
        want = align(alone, sub_batch(b, rest))
        alone.close()
        assert got.counters[:11] == want.counters[:11] and got.extra[:6] == want.extra[:6]
    else:
        assert got.counters[:11] == [0] * 11 and got.extra[:6] == [0] * 6


def test_second_batch_served_from_first(ref, db, ab):
    c = remembering(db)
    info = c.memo_info()
    assert info["entries"] == 0 and info["times_emptied"] == 0 and info["capacity"] > len(ab.keys_a | ab.keys_b)
    got_a = align(c, ab.a)
    check_served(got_a, ab.plain_a, ab.a, set(), db)
    assert got_a.remembered == 0 and c.memo_info()["entries"] == len(ab.keys_a)
    got_b = align(c, ab.b)
    check_served(got_b, ab.plain_b, ab.b, ab.keys_a, db)
    assert got_b.remembered == ab.remembered_b and ab.plain_b.remembered == 0 and ab.plain_b.copies == 0
    info = c.memo_info()
    assert info["entries"] == len(ab.keys_a | ab.keys_b) <= info["capacity"] and 0 < info["bytes_used"] <= MEMO and info["times_emptied"] == 0
    rng = np.random.default_rng(0x3E36)
    hits = [q for q in first_occurrences(ab.b) if key_of(ab.b, q) in ab.keys_a][:60]
    oracle_sample_equal(ref, ab.b, got_b, sorted(set(rng.choice(ab.b.nq, 140, replace=False).tolist()) | set(hits)))
    c.close()


def test_more_than_one_compaction_block(ref, db):
    """9 000 queries = two full blocks of 4 096 and a partial one for the count / scan / compact kernels; a third were seen before."""
    seen = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 3_000, seed=0x3E40)[0]]
    new = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 5_700, seed=0x3E41)[0]]
    rng = np.random.default_rng(0x3E42)
    mixed = seen + new + [new[int(k)] for k in rng.integers(len(new), size=300)]
    first, b = batch_of(seen), batch_of([mixed[i] for i in rng.permutation(len(mixed))])
    assert b.nq == 9_000
    c, plain = remembering(db), db.new_context()
    align(c, first)
    check_served(align(c, b), align(plain, b), b, keys_of(first), db)
    assert c.memo_info()["entries"] == len(keys_of(first) | keys_of(b))
    c.close(); plain.close()


def test_nothing_left_to_align(ref, db, ab):
    c = remembering(db)
    align(c, ab.a)
    again = align(c, ab.a)
    assert again.counters[0] == 0 and again.remembered == len(ab.keys_a) and again.copies == expected_copies(ab.a)
    assert streams_equal(again, ab.plain_a), first_difference(again, ab.plain_a, ab.a.nq)
    assert again.counters[:11] == [0] * 11
    q_hit = first_occurrences(ab.a)[7]
    new = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 1, seed=0x3E50)[0]]
    plain = db.new_context()
    for b, remembered in ((sub_batch(ab.a, [q_hit]), 1), (batch_of(new), 0), (batch_of(new), 1)):
        got = align(c, b)
        assert streams_equal(got, align(plain, b)) and got.remembered == remembered and got.counters[0] == 1 - remembered
    assert len(align(c, batch_of([]))) == 0
    assert c.memo_info()["entries"] == len(ab.keys_a) + 1
    c.close(); plain.close()


def test_long_reads_and_unaligned_results(ref, db):
    """Mates over 320 bases run the long-read passes with the rejection filter; random queries align nowhere (one component, no alignments, no doubles)."""
    long_reads = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 150, read_len=1000, seed=0x3E60)[0]]
    b = batch_of(long_reads + random_queries(100, 150, 0x3E61) + random_queries(100, 1000, 0x3E62))
    c, plain = remembering(db), db.new_context()
    want = align(plain, b)
    assert unaligned_count(want) >= 200 and want.extra[3] == 1
    first, second = align(c, b), align(c, b)
    assert streams_equal(first, want) and first.remembered == 0 and first.counters[0] == b.nq
    assert streams_equal(second, first), first_difference(second, first, b.nq)
    assert second.remembered == b.nq and second.counters[0] == 0 and unaligned_count(second) == unaligned_count(want)
    c.close(); plain.close()


def test_other_parameters_empty_the_memory(db, ab):
    other = api.AlignmentParameters(MaxErrorRate=0.05)
    c, plain = remembering(db), db.new_context()
    align(c, ab.a)
    emptied = c.memo_info()["times_emptied"]
    want = align(plain, ab.a, other)
    got = align(c, ab.a, other)
    assert got.remembered == 0 and c.memo_info()["times_emptied"] == emptied + 1
    assert streams_equal(got, want), first_difference(got, want, ab.a.nq)
    assert not streams_equal(want, ab.plain_a)  # (the parameter matters to these reads)
    again = align(c, ab.a, other)
    assert again.remembered == len(ab.keys_a) and again.counters[0] == 0 and streams_equal(again, want)
    assert c.memo_info()["times_emptied"] == emptied + 1 and c.memo_info()["entries"] == len(ab.keys_a)
    c.close(); plain.close()


def test_budget(ref, db, ab):
    c = db.new_context()
    with pytest.raises(RuntimeError):
        c.set_memo(MIN_MEMO - 1)
    c.set_memo(MIN_MEMO)
    capacity = c.memo_info()["capacity"]
    assert 0 < capacity < len(ab.keys_a)  # A does not fit
    got = align(c, ab.a)
    assert streams_equal(got, ab.plain_a) and got.remembered == 0
    entries = c.memo_info()["entries"]
    assert 0 < entries <= capacity and c.memo_info()["bytes_used"] <= MIN_MEMO
    third = batch_of(duplicated(mixed_distinct(ref, 900, 300, seed=0x3E70), seed=0x3E71))
    plain = db.new_context()
    held = set(ab.keys_a)
    for b, want in ((ab.b, ab.plain_b), (third, align(plain, third)), (ab.a, ab.plain_a)):
        got = align(c, b)
        assert streams_equal(got, want), first_difference(got, want, b.nq)
        assert 0 <= got.remembered <= min(entries, expected_remembered(b, held)) and got.copies == expected_copies(b)
        assert got.counters[0] == b.nq - got.remembered - got.copies
        assert c.memo_info()["entries"] == entries  # full: nothing more is remembered
        held |= keys_of(b)
    assert got.remembered > 0  # (A again: what did fit is served)
    c.close()
    # switched off, the memory is back with the GPU and a call launches what a call of a context that never had one launches
    se = batch_of([([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 2_000, seed=0x3E72)[0]])
    c = db.new_context()
    launches = align(c, se).kernel_launches
    free_before = api.device_memory(0)[0]
    c.set_memo(MEMO)
    assert api.device_memory(0)[0] <= free_before - (MEMO - (1 << 20))
    on = align(c, se)
    assert on.kernel_launches > launches and c.memo_info()["entries"] == len(keys_of(se))
    c.set_memo(0)
    assert api.device_memory(0)[0] == free_before
    off = align(c, se)
    assert off.kernel_launches == launches == align(plain, se).kernel_launches and off.remembered == 0 and off.counters[0] == se.nq
    assert c.memo_info()["entries"] == 0 and c.memo_info()["bytes_used"] == 0
    c.close(); plain.close()


def test_fingerprint_collisions(db, ab, monkeypatch):
    """Six bits of fingerprint: thousands of different queries share 63 keys, so the header and byte comparison of the lookup and the drop of the insert decide."""
    monkeypatch.setenv("XM_MEMO_FINGERPRINT_BITS", "6")
    c = remembering(db)
    got_a, got_b = align(c, ab.a), align(c, ab.b)
    assert streams_equal(got_a, ab.plain_a), first_difference(got_a, ab.plain_a, ab.a.nq)
    assert streams_equal(got_b, ab.plain_b), first_difference(got_b, ab.plain_b, ab.b.nq)
    assert got_a.remembered == 0 and 0 <= got_b.remembered <= ab.remembered_b and got_b.copies == expected_copies(ab.b)
    assert 0 < c.memo_info()["entries"] <= 63
    again = align(c, ab.a)
    assert streams_equal(again, ab.plain_a) and 0 < again.remembered <= 63
    c.close()


def test_memory_survives_growth_of_the_tables(ref, ab):
    """Tables hashed up to 150 bases; a batch with 400-base reads grows them.  What was remembered before is served after: a read only reads the tables of
    lengths up to its own."""
    small = api.ReferenceDatabase([("syn", ref)], max_query_length=150)
    hashed = small.info()["max_hashed_length"]
    c = small.new_context()
    c.set_memo(MEMO)
    align(c, ab.a)
    longer = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 300, read_len=400, seed=0x3E80)[0]]
    firsts = first_occurrences(ab.a)
    b = batch_of(sub_batch_queries(ab.a, firsts) + longer)
    got = align(c, b)
    assert small.info()["max_hashed_length"] > hashed >= 150
    assert got.remembered == len(firsts) and got.counters[0] == b.nq - got.remembered - got.copies
    plain = small.new_context()
    want = align(plain, b)
    assert streams_equal(got, want), first_difference(got, want, b.nq)
    c.close(); plain.close(); small.close()


def sub_batch_queries(b, idx):
    return [([np.array(b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]]) for m in range(int(b.mate_count[q]))],
             float(b.expected_inner[q]), float(b.deviation[q])) for q in idx]


def test_wave_form(db, ab, monkeypatch):
    monkeypatch.setenv("XM_WAVE", "1")
    c = remembering(db)
    got_a, got_b = align(c, ab.a), align(c, ab.b)
    assert streams_equal(got_a, ab.plain_a), first_difference(got_a, ab.plain_a, ab.a.nq)
    assert streams_equal(got_b, ab.plain_b), first_difference(got_b, ab.plain_b, ab.b.nq)
    assert got_b.remembered == ab.remembered_b and got_b.copies == expected_copies(ab.b) and got_b.counters[0] + got_b.remembered + got_b.copies <= ab.b.nq
    c.close()


def test_streaming_and_two_contexts(ref, db, ab):
    batches, plains = (ab.a, ab.b, ab.a, ab.b), (ab.plain_a, ab.plain_b, ab.plain_a, ab.plain_b)
    arrays = [arrays_of(x) for x in batches]
    c = remembering(db)
    got = list(c.align_stream(iter(arrays), PARAMS))
    for x, g, w in zip(batches, got, plains):
        assert streams_equal(g, w), first_difference(g, w, x.nq)
    assert got[1].remembered == ab.remembered_b
    for x, g in zip(batches[2:], got[2:]):
        assert g.remembered == len(keys_of(x)) and g.counters[0] == 0 and g.copies == expected_copies(x)
    c.close()
    two = multi.MultiGpuDatabase([("syn", ref)], [0, 0], memo_bytes=MEMO)  # batch k goes to context k mod 2: each context sees one batch twice
    got = list(two.align_stream(iter(arrays), PARAMS))
    for x, g, w in zip(batches, got, plains):
        assert streams_equal(g, w), first_difference(g, w, x.nq)
    assert got[0].remembered == 0 and got[1].remembered == 0
    for x, g in zip(batches[2:], got[2:]):
        assert g.remembered == len(keys_of(x)) and g.counters[0] == 0
    two.close()


def test_pileup_after_served_batch(ref, db):
    """xm_pileup_add_last reads the canonical streams: a batch served from the memory piles up exactly as the aligned one (depth, alternatives, middle depth, events)."""
    reads = synth.synthetic_single_end(ref, 1_500, seed=0x3E90, indel_prob=0.3)[0]
    m1, m2 = synth.synthetic_paired_end(ref, 500, seed=0x3E91, indel_prob=0.3)[:2]
    distinct = [api.Query(x) for x in reads] + [api.Query(m1[i], m2[i], expected_inner_distance=100.0, spacing_deviation_per_unit_penalty=50.0) for i in range(len(m1))]
    queries = duplicated(distinct, seed=0x3E92)
    piles = []
    for remember in (False, True):
        c = db.new_context()
        if remember:
            c.set_memo(MEMO)
            c.align_batch(queries, PARAMS)
        res = c.align_batch(queries, PARAMS)
        assert res.remembered == (len(distinct) if remember else 0) and res.counters[0] == (0 if remember else len(queries))
        m = pileup.MatchDatabase(c, 0.1)
        n_events = m.add_last(queries)
        depth, alt = m._sum(0)
        piles.append((n_events, depth, alt, m._middle(0), m._events(), m.mutations()))
        m.close(); c.close()
    (n0, d0, a0, mid0, e0, mu0), (n1, d1, a1, mid1, e1, mu1) = piles
    assert n0 == n1 > 100 and np.array_equal(d0, d1) and np.array_equal(a0, a1) and np.array_equal(mid0, mid1) and e0 == e1 and mu0 == mu1


def test_cli_remember_queries(ref, tmp_path):
    """python -m mapper_amd with and without --remember-queries: byte-identical outputs, one statistics line on stderr."""
    small = ref[:400_000]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(small) + "\n")
    reads = synth.synthetic_single_end(small, 1_500, seed=0x3EA0, indel_prob=0.3)[0]
    rng = np.random.default_rng(0x3EA1)
    picks = rng.choice(len(reads), 4_000)
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, k in enumerate(picks):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(reads[k]), "I" * len(reads[k])))
    env = dict(os.environ)
    env["PYTHONNOUSERSITE"] = "1"

    def run(tag, extra):
        outs = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("sam", "unaligned")}
        argv = [sys.executable, "-m", "mapper_amd", "--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--out-sam", outs["sam"],
                "--out-unaligned", outs["unaligned"], "--batch-size", "1000"]
        r = subprocess.run(argv + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return {k: open(v, "rb").read() for k, v in outs.items()}, r

    plain, rp = run("plain", [])
    got, rg = run("memo", ["--remember-queries", "64"])
    assert plain == got and len(got["sam"]) > 100_000
    assert "Remembered queries" not in rp.stderr
    line = [l for l in rg.stderr.splitlines() if l.startswith("Remembered queries")]
    assert len(line) == 1 and int(line[0].split()[2]) > 0 and " of 4000 " in line[0], rg.stderr[-2000:]
    assert rp.stdout == rg.stdout
