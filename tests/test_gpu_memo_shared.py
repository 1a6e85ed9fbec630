"""GPU tier: one memory of aligned queries per GPU, shared by its contexts and never full (xm_memory_new, xm_context_attach_memory; api.QueryMemory,
ReferenceDatabase.attach_memory, MultiGpuDatabase(shared_memo_bytes=), --remember-queries-per-gpu).  The invariant of tests/test_gpu_memo.py is untouched - a
query is only ever served from a byte-identical query aligned earlier under bit-identical parameters, so the four streams never change - and the amount of work
follows the rules of mapper_amd/csrc/xm_memo_plan.h: expected counts come from the queries' keys (memo_helpers), record bytes from the plain context's result
offsets with the layout that header states, turns and promotions from the model below."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from helpers import streams_equal, first_difference
from memo_helpers import PARAMS, align, arrays_of, batch_of, duplicated, expected_copies, expected_remembered, first_occurrences, key_of, keys_of
from test_gpu_memo import Pair, ab, db, ref  # noqa: F401  (the 1 Mb synthetic reference, its database and the two batches A and B of that file, as fixtures here)
from mapper_amd import api, multi, pileup, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 64 << 20
MIN_MEMO = 64 << 10
GEN_ARENA, GEN_CAPACITY = 49_152, 512  # memoPlan(64 KiB): 1 024 slots of 16 bytes, the rest for the records; half the slots are ever claimed


def pad8(n):
    return (n + 7) & ~7


def record_bytes(b, plain, q):
    """xm_memo_plan.h: a header of 40 bytes, the mates' bytes, the int slice, the double slice, every part padded to a multiple of 8"""
    mates = int(b.mate_length[2 * q]) + (int(b.mate_length[2 * q + 1]) if b.mate_count[q] > 1 else 0)
    return 40 + pad8(mates) + pad8(4 * int(plain.int_off[q + 1] - plain.int_off[q])) + 8 * int(plain.dbl_off[q + 1] - plain.dbl_off[q])


def records_of(b, plain):
    """key -> record bytes of b's distinct queries"""
    return {key_of(b, q): record_bytes(b, plain, q) for q in first_occurrences(b)}


class Generations:
    """The rules of xm_memo_plan.h for batches that each fit a generation (what these tests run): key -> bytes per generation."""

    def __init__(self, generations=2, arena=GEN_ARENA, capacity=GEN_CAPACITY):
        self.arena, self.capacity, self.generations = arena, capacity, generations
        self.young, self.old = {}, {}
        self.turns = self.promoted = 0

    def takes(self, recs):
        return len(self.young) + len(recs) <= self.capacity and sum(self.young.values()) + sum(recs.values()) <= self.arena

    def call(self, recs):
        """-> (served from the young generation, served from the old one) for a call with these distinct queries"""
        from_young = {k for k in recs if k in self.young}
        from_old = {k: v for k, v in recs.items() if k not in self.young and k in self.old}
        if self.generations == 2 and from_old and self.takes(from_old):
            self.young.update(from_old)
            self.promoted += len(from_old)
        misses = {k: v for k, v in recs.items() if k not in from_young and k not in from_old}
        if misses:
            if self.generations == 2 and self.young and not self.takes(misses):
                self.old, self.young = self.young, {}
                self.turns += 1
            assert self.generations == 1 or self.takes(misses)  # (the model is for batches that fit)
            if self.takes(misses):
                self.young.update(misses)
        return len(from_young), len(from_old)


@pytest.fixture(scope="module")
def reads(ref, db):  # noqa: F811
    """1 800 different single reads of 150 bases, what a plain context returns for them, and each one's record bytes"""
    s = Pair()
    s.queries = [([r], 0.0, 1.0) for r in synth.synthetic_single_end(ref, 1_800, seed=0x3F20)[0]]
    s.batch = batch_of(s.queries)
    assert len(keys_of(s.batch)) == 1_800
    plain = db.new_context()
    s.plain = align(plain, s.batch)
    plain.close()
    s.bytes = [record_bytes(s.batch, s.plain, q) for q in range(s.batch.nq)]
    return s


def batches_of(db, reads, n, count):  # noqa: F811
    """`count` batches of n consecutive reads: [(batch, plain result, key -> record bytes)]"""
    out = []
    plain = db.new_context()
    for k in range(count):
        b = batch_of(reads.queries[k * n:(k + 1) * n])
        want = align(plain, b)
        recs = records_of(b, want)
        assert sorted(recs.values()) == sorted(reads.bytes[k * n:(k + 1) * n])
        out.append((b, want, recs))
    plain.close()
    return out


def attached(d, memory):
    c = d.new_context()
    c.attach_memory(memory)
    return c


def same(got, want, b):
    assert streams_equal(got, want), first_difference(got, want, b.nq)
    assert got.counters[0] + got.remembered + got.copies == b.nq


def test_two_contexts_one_memory_in_turn(db, ab):  # noqa: F811
    memory = api.QueryMemory(db, BIG)
    ca, cb = attached(db, memory), attached(db, memory)
    info = memory.info()
    assert info["contexts"] == 2 and info["generations"] == 2 and info["entries"] == 0 and info["turns"] == 0 and info["capacity"] > len(ab.keys_a | ab.keys_b)
    got = align(ca, ab.a)
    same(got, ab.plain_a, ab.a)
    assert got.remembered == 0 and memory.info()["entries"] == len(ab.keys_a)
    got = align(cb, ab.a)  # B has aligned nothing yet: all of A's work serves it
    same(got, ab.plain_a, ab.a)
    assert got.remembered == len(ab.keys_a) and got.counters[0] == 0 and got.copies == expected_copies(ab.a)
    got = align(cb, ab.b)
    same(got, ab.plain_b, ab.b)
    assert got.remembered == expected_remembered(ab.b, ab.keys_a) == ab.remembered_b
    info = memory.info()
    assert info["contexts"] == 2 and info["entries"] == len(ab.keys_a | ab.keys_b) and info["turns"] == 0 and info["promoted"] == 0 and info["times_emptied"] == 0
    # one copy of the records: the bytes in use are what ONE per-context memory of the same plan uses for the same batches (two generations of BIG / 2 have the
    # tables of one memory of BIG / 2 twice; the records are the same bytes), not twice that
    alone = db.new_context()
    alone.set_memo(BIG // 2)
    align(alone, ab.a), align(alone, ab.b)
    one = alone.memo_info()
    tables = 16 * 2 * one["capacity"]
    assert one["entries"] == info["entries"] and info["bytes_used"] - 2 * tables == one["bytes_used"] - tables > 0
    assert ca.memo_info() == {"entries": 0, "bytes_used": 0, "capacity": 0, "times_emptied": 0}  # (the context has no memory of its own)
    alone.close(); ca.close(); cb.close()
    assert memory.info()["contexts"] == 0
    memory.close()


def run_sequence(c, memory, model, steps):
    """steps: (batch, plain result, records) in order -> [(remembered, served from young, served from old by the model)]"""
    out = []
    for b, want, recs in steps:
        got = align(c, b)
        same(got, want, b)
        y, o = model.call(recs)
        out.append((got.remembered, y, o))
        info = memory.info()
        assert info["turns"] == model.turns and info["promoted"] == model.promoted, (len(out), info, model.turns, model.promoted)
    return out


def test_it_keeps_remembering(db, reads):  # noqa: F811
    """2 x 64 KiB: a generation holds 49 152 bytes of records.  One batch fits a generation and two do not, so every new batch turns the generations: the last
    two batches are always held, however long the run is.  One generation of the same total budget stops after its first batches."""
    n = min(GEN_ARENA // max(reads.bytes), GEN_CAPACITY)
    bs = batches_of(db, reads, n, 6)
    sizes = [sum(r.values()) for _, _, r in bs]
    assert all(s <= GEN_ARENA for s in sizes) and n <= GEN_CAPACITY                      # one batch fits a generation
    assert all(sizes[i] + sizes[j] > GEN_ARENA for i in range(6) for j in range(i))      # two do not
    memory = api.QueryMemory(db, 2 * MIN_MEMO, generations=2)
    with pytest.raises(RuntimeError):
        api.QueryMemory(db, 2 * MIN_MEMO - 1, generations=2)
    c = attached(db, memory)
    model = Generations()
    served = run_sequence(c, memory, model, bs + [bs[5], bs[4], bs[0]])
    assert [s[0] for s in served[:6]] == [0] * 6
    assert served[6] == (n, n, 0)   # batch 6: wholly remembered
    assert served[7] == (n, 0, n)   # batch 5: wholly remembered, from the old generation (the young one is full: no second chance)
    assert served[8] == (0, 0, 0)   # batch 1: gone long ago
    assert model.turns == 6 and memory.info()["turns"] == 6 and memory.info()["entries"] == 2 * n
    c.close(); memory.close()
    # one generation of the same total budget: 98 304 bytes of records take two batches and a piece of the third; then full means it stops
    memory = api.QueryMemory(db, 2 * MIN_MEMO, generations=1)
    c = attached(db, memory)
    entries = []
    for b, want, _ in bs:
        same(align(c, b), want, b)
        entries.append(memory.info()["entries"])
    assert entries[3] == entries[4] == entries[5] and 2 * n <= entries[3] < 4 * n and entries[0] == n  # it stops growing after the fourth batch at the latest
    got = align(c, bs[5][0])
    same(got, bs[5][1], bs[5][0])
    assert got.remembered == 0 and memory.info()["turns"] == 0 and memory.info()["generations"] == 1
    assert align(c, bs[0][0]).remembered == n  # (what did fit is served)
    c.close(); memory.close()


def test_second_chance(db, reads):  # noqa: F811
    """Three batches fit a generation and four do not.  b1 comes back while it is in the old generation, is served from there and copied into the young one;
    at the next turn b1 is still held, b2 and b3 - as old as b1, never asked for again - are gone."""
    n = min(GEN_ARENA // (3 * max(reads.bytes)), GEN_CAPACITY // 3)
    bs = batches_of(db, reads, n, 6)
    sizes = sorted(sum(r.values()) for _, _, r in bs)
    assert sum(sizes[-3:]) <= GEN_ARENA and 3 * n <= GEN_CAPACITY   # any three fit
    assert sum(sizes[:4]) > GEN_ARENA                               # no four do
    b1, b2, b3, b4, b5, b6 = bs
    memory = api.QueryMemory(db, 2 * MIN_MEMO)
    c = attached(db, memory)
    model = Generations()
    served = run_sequence(c, memory, model, [b1, b2, b3, b4, b1, b5, b6])
    assert [s[0] for s in served] == [0, 0, 0, 0, n, 0, 0] and served[4] == (n, 0, n)
    assert model.turns == 2 and model.promoted == n
    served = run_sequence(c, memory, model, [b1, b2, b3])
    assert served[0] == (n, 0, n)                     # b1: wholly remembered (and promoted once more)
    assert served[1][0] == 0 and served[2][0] == 0    # b2, b3: not at all
    assert memory.info()["promoted"] == n * 2 == model.promoted
    c.close(); memory.close()


def test_one_fingerprint_two_queries_two_generations(db, ab, monkeypatch):  # noqa: F811
    """Six bits of fingerprint and generations of 64 KiB: 63 keys a generation, thousands of queries a call, so every call that aligned something turns the
    generations, and lookups meet other queries' records in both of them."""
    monkeypatch.setenv("XM_MEMO_FINGERPRINT_BITS", "6")
    memory = api.QueryMemory(db, 2 * MIN_MEMO)
    monkeypatch.delenv("XM_MEMO_FINGERPRINT_BITS")
    c = attached(db, memory)
    held = set()
    for b, want in ((ab.a, ab.plain_a), (ab.b, ab.plain_b), (ab.a, ab.plain_a), (ab.b, ab.plain_b), (ab.a, ab.plain_a)):
        got = align(c, b)
        same(got, want, b)
        assert 0 <= got.remembered <= expected_remembered(b, held) and got.copies == expected_copies(b)
        held |= keys_of(b)
        assert 0 < memory.info()["entries"] <= 2 * 63
    assert memory.info()["turns"] >= 3
    c.close(); memory.close()


def test_other_parameters_through_the_other_context(db, ab):  # noqa: F811
    other = api.AlignmentParameters(MaxErrorRate=0.05)
    memory = api.QueryMemory(db, BIG)
    ca, cb, plain = attached(db, memory), attached(db, memory), db.new_context()
    same(align(ca, ab.a), ab.plain_a, ab.a)
    emptied = memory.info()["times_emptied"]
    want = align(plain, ab.a, other)
    got = align(cb, ab.a, other)
    assert got.remembered == 0 and memory.info()["times_emptied"] == emptied + 1
    same(got, want, ab.a)
    assert not streams_equal(want, ab.plain_a)  # (the parameter matters to these reads)
    again = align(ca, ab.a, other)              # what B aligned under the other parameters serves A
    same(again, want, ab.a)
    assert again.remembered == len(ab.keys_a) and again.counters[0] == 0
    assert memory.info()["times_emptied"] == emptied + 1 and memory.info()["entries"] == len(ab.keys_a)
    ca.close(); cb.close(); plain.close(); memory.close()


def test_side_by_side(db, ab):  # noqa: F811
    memory = api.QueryMemory(db, BIG)
    ctx = [attached(db, memory), attached(db, memory)]
    results, errors = [[], []], []

    def work(k):
        try:
            for b in (ab.a, ab.b, ab.a, ab.b):
                results[k].append(align(ctx[k], b))
        except BaseException as e:  # noqa: BLE001  (handed to the test)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert len(results[k]) == 4
        for got, b, want in zip(results[k], (ab.a, ab.b, ab.a, ab.b), (ab.plain_a, ab.plain_b, ab.plain_a, ab.plain_b)):
            same(got, want, b)
        assert results[k][2].remembered == len(ab.keys_a) and results[k][3].remembered == len(ab.keys_b)  # (the context's own first two calls, at the least)
    for c in ctx:
        for b, want in ((ab.a, ab.plain_a), (ab.b, ab.plain_b)):
            got = align(c, b)
            same(got, want, b)
            assert got.remembered == len(keys_of(b)) and got.counters[0] == 0
    info = memory.info()
    assert info["entries"] == len(ab.keys_a | ab.keys_b) and info["turns"] == 0  # (the records held do not exceed the distinct keys: a key both aligned is held once)
    for c in ctx:
        c.close()
    memory.close()


def test_lifetime_and_errors(ref, db, ab):  # noqa: F811
    ca, cb = db.new_context(), db.new_context()
    # (the contexts' own buffers first, at sizes no later call outgrows: a served batch needs room for the remembered slices on top)
    warm = batch_of([q for _ in range(4) for q in _queries_of(ab.a)])
    assert 3 * ab.a.nq * 40 >= len(ab.plain_a.ints) and 3 * ab.a.nq * 12 >= len(ab.plain_a.dbls)
    for c in (ca, cb):
        align(c, warm)
    free_before = api.device_memory(0)[0]
    # errors: each fails with a message and changes nothing
    for nbytes, generations in ((2 * MIN_MEMO - 1, 2), (MIN_MEMO - 1, 1), (BIG, 0), (BIG, 3), (-1, 2)):
        with pytest.raises(RuntimeError) as e:
            api.QueryMemory(db, nbytes, generations)
        assert "xm_memory_new" in str(e.value)
    memory = api.QueryMemory(db, BIG)
    assert api.device_memory(0)[0] <= free_before - (BIG - (1 << 20))
    elsewhere = api.ReferenceDatabase([("other", ref[:50_000])])
    host = api.ReferenceDatabase([("other", ref[:50_000])], host_only=True)
    own = db.new_context()
    own.set_memo(MIN_MEMO)
    for c, word in ((elsewhere, "another index"), (host, "host_only"), (own, "of its own")):
        with pytest.raises(RuntimeError) as e:
            c.attach_memory(memory)
        assert word in str(e.value), str(e.value)
    with pytest.raises(RuntimeError) as e:
        api.QueryMemory(host, BIG)
    assert "host_only" in str(e.value)
    assert own.memo_info()["capacity"] > 0 and memory.info()["contexts"] == 0
    own.set_memo(0)
    own.attach_memory(memory)
    with pytest.raises(RuntimeError) as e:
        own.set_memo(MIN_MEMO)  # a memory of its own on an attached context
    assert "attached" in str(e.value) and memory.info()["contexts"] == 1
    own.close(); elsewhere.close(); host.close()
    assert memory.info()["contexts"] == 0
    # the handle goes first: the contexts keep being served
    ca.attach_memory(memory); cb.attach_memory(memory)
    ca.attach_memory(memory)  # (again: nothing changes)
    assert memory.info()["contexts"] == 2
    same(align(ca, ab.a), ab.plain_a, ab.a)
    memory.close()
    got = align(cb, ab.a)
    same(got, ab.plain_a, ab.a)
    assert got.remembered == len(ab.keys_a)
    assert api.device_memory(0)[0] < free_before
    ca.attach_memory(None)
    got = align(ca, ab.a)  # detached: a plain context again
    assert got.remembered == 0 and got.copies == 0 and got.counters[0] == ab.a.nq and streams_equal(got, ab.plain_a)
    assert align(cb, ab.a).remembered == len(ab.keys_a)
    cb.attach_memory(None)
    assert api.device_memory(0)[0] == free_before  # all of its HBM is back
    # the contexts go first, one detached and one closed while attached; then the handle
    memory = api.QueryMemory(db, BIG, generations=1)
    cc = attached(db, memory)
    ca.attach_memory(memory)
    same(align(ca, ab.a), ab.plain_a, ab.a)
    assert align(cc, ab.a).remembered == len(ab.keys_a)
    cc.close()
    ca.attach_memory(None)
    assert memory.info()["contexts"] == 0 and memory.info()["entries"] == len(ab.keys_a)
    assert api.device_memory(0)[0] <= free_before - (BIG - (1 << 20))
    memory.close()
    assert api.device_memory(0)[0] == free_before
    ca.close(); cb.close()


def _queries_of(b):
    return [([np.array(b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]]) for m in range(int(b.mate_count[q]))],
             float(b.expected_inner[q]), float(b.deviation[q])) for q in range(b.nq)]


def test_multi_gpu_database_shares_one_memory_per_gpu(ref, ab):  # noqa: F811
    batches, plains = (ab.a, ab.b, ab.b, ab.a), (ab.plain_a, ab.plain_b, ab.plain_b, ab.plain_a)
    with pytest.raises(ValueError):
        multi.MultiGpuDatabase([("syn", ref)], [0, 0], memo_bytes=BIG, shared_memo_bytes=BIG)
    two = multi.MultiGpuDatabase([("syn", ref)], [0, 0], shared_memo_bytes=BIG)
    assert len(two.memories) == 1 and two.memories[0].info()["contexts"] == 2 and two.memories[0].info()["generations"] == 2
    got = list(two.align_stream(iter([arrays_of(x) for x in batches]), PARAMS))
    for x, g, w in zip(batches, got, plains):
        same(g, w, x)
    # batch k goes to context k mod 2: the third batch (B, on the context that aligned A) is served A's part at the least - what a per-context memory would give -
    # and whatever of B the other context had remembered by then; the fourth (A, on the context that aligned B) is wholly remembered
    assert got[2].remembered >= expected_remembered(ab.b, ab.keys_a)
    assert got[3].remembered == len(ab.keys_a) and got[3].counters[0] == 0
    assert two.memories[0].info()["entries"] <= len(ab.keys_a | ab.keys_b)
    memory = two.memories[0]
    two.close()
    assert two.memories == [] and memory._h is None


def test_cli_remember_queries_per_gpu(ref, tmp_path):  # noqa: F811
    """python -m mapper_amd with two contexts: byte-identical outputs with and without --remember-queries-per-gpu, one statistics line on stderr, and at least
    as many queries served as with a memory per context."""
    small = ref[:400_000]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(small) + "\n")
    distinct = synth.synthetic_single_end(small, 500, seed=0x3F30, indel_prob=0.3)[0]
    picks = np.random.default_rng(0x3F31).choice(len(distinct), 1_500)
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, k in enumerate(picks):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(distinct[k]), "I" * len(distinct[k])))
    env = dict(os.environ)
    env["PYTHONNOUSERSITE"] = "1"

    def run(tag, extra):
        outs = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("sam", "unaligned")}
        argv = [sys.executable, "-m", "mapper_amd", "--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--out-sam", outs["sam"],
                "--out-unaligned", outs["unaligned"], "--batch-size", "400", "--contexts", "2"]
        r = subprocess.run(argv + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stderr.splitlines() if l.startswith("Remembered queries")]
        return {k: open(v, "rb").read() for k, v in outs.items()}, r, lines

    plain, rp, none = run("plain", [])
    shared, rs, line_s = run("shared", ["--remember-queries-per-gpu", "8"])
    each, re_, line_e = run("each", ["--remember-queries", "8"])
    assert plain == shared == each and len(plain["sam"]) > 50_000 and rp.stdout == rs.stdout
    assert none == [] and len(line_s) == 1 and len(line_e) == 1 and " of 1500 " in line_s[0]
    assert int(line_s[0].split()[2]) >= int(line_e[0].split()[2]) > 0, (line_s, line_e)
    both = subprocess.run([sys.executable, "-m", "mapper_amd", "--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--no-output",
                           "--remember-queries", "8", "--remember-queries-per-gpu", "8"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert both.returncode == 1 and "exclude each other" in both.stderr


def test_pileup_after_a_batch_served_from_a_promoted_record(ref, db):  # noqa: F811
    """As test_gpu_memo.test_pileup_after_served_batch, with the batch served through a shared two-generation memory from records that were promoted: they went
    into the old generation at a turn, were served from there and copied into the young one, and the pile-up reads the batch that copy serves."""
    reads_ = synth.synthetic_single_end(ref, 60, seed=0x3F40, indel_prob=0.3)[0]
    m1, m2 = synth.synthetic_paired_end(ref, 10, seed=0x3F41, indel_prob=0.3)[:2]
    distinct = [api.Query(x) for x in reads_] + [api.Query(m1[i], m2[i], expected_inner_distance=100.0, spacing_deviation_per_unit_penalty=50.0) for i in range(len(m1))]
    queries = duplicated(distinct, seed=0x3F42)
    # records of single reads of 150 bases with one alignment are 288 - 320 bytes, of pairs 480 - 544: the queries are at most 24 640 bytes, each filler of 60 single
    # reads 17 280 - 19 200.  Filler, queries and filler do not fit a generation of 49 152 bytes (>= 56 640): the second filler turns the generations.  The second
    # filler and the queries do (<= 43 840): the queries are promoted.  (The counts asserted below say whether it went so.)
    filler = [api.Query(x) for x in synth.synthetic_single_end(ref, 120, seed=0x3F43)[0]]
    piles = []
    for remember in (False, True):
        c = db.new_context()
        if remember:
            memory = api.QueryMemory(db, 2 * MIN_MEMO)
            c.attach_memory(memory)
            c.align_batch(filler[:60], PARAMS)
            c.align_batch(queries, PARAMS)        # into the young generation, beside the first filler
            assert memory.info()["turns"] == 0 and memory.info()["entries"] == 60 + len(distinct)
            c.align_batch(filler[60:], PARAMS)    # does not fit beside them: a turn, the queries are in the old generation now
            assert memory.info()["turns"] == 1 and memory.info()["promoted"] == 0
            res = c.align_batch(queries, PARAMS)  # served from the old generation, and promoted
            assert res.remembered == len(distinct) and memory.info()["promoted"] == len(distinct) and memory.info()["turns"] == 1
        res = c.align_batch(queries, PARAMS)      # with the memory: served from the promoted records in the young generation
        assert res.remembered == (len(distinct) if remember else 0) and res.counters[0] == (0 if remember else len(queries))
        if remember:
            assert memory.info()["promoted"] == len(distinct)  # (nothing was promoted again: the young generation served it)
        m = pileup.MatchDatabase(c, 0.1)
        n_events = m.add_last(queries)
        depth, alt = m._sum(0)
        piles.append((n_events, depth, alt, m._middle(0), m._events(), m.mutations()))
        m.close(); c.close()
        if remember:
            memory.close()
    (n0, d0, a0, mid0, e0, mu0), (n1, d1, a1, mid1, e1, mu1) = piles
    assert n0 == n1 > 10 and np.array_equal(d0, d1) and np.array_equal(a0, a1) and np.array_equal(mid0, mid1) and e0 == e1 and mu0 == mu1
