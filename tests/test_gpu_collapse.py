"""GPU tier: identical queries of a batch aligned once (xm_context_set_collapse, api.ReferenceDatabase.set_collapse; the reference's
AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291, within a batch).  The streams must not change, the work counters count the
representatives only, and xm_result.extra[7] the queries served as copies."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as o
from helpers import streams_equal, first_difference
from mapper_amd import api, multi, pileup, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = api.AlignmentParameters()


@pytest.fixture(scope="module")
def ref():
    return synth.synthetic_reference(5_000_000, seed=0xC011A)


@pytest.fixture(scope="module")
def db(ref):
    d = api.ReferenceDatabase([("syn", ref)])
    yield d
    d.close()


def batch_of(queries, shared=()):
    """queries: list of (mates, expected_inner, deviation) -> QueryBatch.  shared: indices of queries appended again, as queries whose mates point at the
    very bytes of `codes` the original's do (the same offsets)."""
    b = o.QueryBatch(queries)
    if not shared:
        return b
    extra = list(shared)
    mc = np.concatenate([b.mate_count, b.mate_count[extra]])
    mo = np.concatenate([b.mate_offset, np.stack([b.mate_offset[0::2][extra], b.mate_offset[1::2][extra]], axis=1).reshape(-1)])
    ml = np.concatenate([b.mate_length, np.stack([b.mate_length[0::2][extra], b.mate_length[1::2][extra]], axis=1).reshape(-1)])
    return o.QueryBatch.from_arrays(mc.astype(np.int32), mo.astype(np.int64), ml.astype(np.int32), b.codes, np.concatenate([b.expected_inner, b.expected_inner[extra]]),
                                    np.concatenate([b.deviation, b.deviation[extra]]))


def key_of(b, q):
    """What a query's alignment reads: mate count, mates (bytes, in order), the bit patterns of expected_inner and deviation."""
    mates = tuple(bytes(b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]]) for m in range(int(b.mate_count[q])))
    return (int(b.mate_count[q]), mates, np.float64(b.expected_inner[q]).view(np.int64).item(), np.float64(b.deviation[q]).view(np.int64).item())


def expected_copies(b):
    return b.nq - len({key_of(b, q) for q in range(b.nq)})


def align(d, b):
    return d.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, PARAMS)


def fresh(d, collapse):
    c = d.new_context()
    c.set_collapse(collapse)
    return c


def duplicated(distinct, seed, counts=(1, 2, 5, 50), p=(0.6, 0.25, 0.13, 0.02)):
    """every query of `distinct` a seeded random number of times, shuffled"""
    rng = np.random.default_rng(seed)
    reps = rng.choice(counts, size=len(distinct), p=p)
    out = [q for q, k in zip(distinct, reps) for _ in range(int(k))]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def first_occurrences(b):
    seen, firsts = set(), []
    for q in range(b.nq):
        k = key_of(b, q)
        if k not in seen:
            seen.add(k)
            firsts.append(q)
    return firsts


def sub_batch(b, idx):
    idx = list(idx)
    return o.QueryBatch([([b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]] for m in range(int(b.mate_count[q]))],
                          float(b.expected_inner[q]), float(b.deviation[q])) for q in idx])


def mixed_distinct(ref, n_se, n_pe, seed, read_len=150):
    se = synth.synthetic_single_end(ref, n_se, read_len=read_len, seed=seed)[0]
    m1, m2 = synth.synthetic_paired_end(ref, n_pe, read_len=read_len, seed=seed + 1)[:2]
    return [([r], 0.0, 1.0) for r in se] + [([m1[i], m2[i]], 100.0, 50.0) for i in range(n_pe)]


def near_copies(distinct, rng):
    """queries that differ from one of `distinct` in one thing each: none of them may be served from it"""
    out = []
    se = [q for q in distinct if len(q[0]) == 1]
    pe = [q for q in distinct if len(q[0]) == 2]
    for k in range(40):
        (r,), e, d = se[int(rng.integers(len(se)))]
        i = int(rng.integers(len(r)))
        changed = r.copy(); changed[i] = {1: 2, 2: 4, 4: 8, 8: 1}.get(int(r[i]), 1)
        n = r.copy(); n[i] = 15
        out += [([changed], e, d), ([n], e, d), ([r[:-1].copy()], e, d), ([r], e + 1.0, d)]
        (a, b), e, d = pe[int(rng.integers(len(pe)))]
        out += [([b, a], e, d), ([a, b], e + 1.0, d), ([a, b], e, d * 2), ([a], 0.0, 1.0), ([a], e, d)]
    return out


def oracle_sample_equal(ref, b, got, idx):
    want = o.OracleReference([("syn", ref)]).align(sub_batch(b, idx), o.make_params())
    for k, q in enumerate(idx):
        gi = got.ints[got.int_off[q]:got.int_off[q + 1]]
        gd = np.asarray(got.dbls[got.dbl_off[q]:got.dbl_off[q + 1]]).view(np.int64)
        wi = want.ints[want.int_off[k]:want.int_off[k + 1]]
        wd = want.dbls[want.dbl_off[k]:want.dbl_off[k + 1]].view(np.int64)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd), "query %d differs from the oracle" % q


def check_output_and_work(ref, d, b, extra3=None):
    on, off = fresh(d, True), fresh(d, False)
    got, plain = align(on, b), align(off, b)
    assert streams_equal(got, plain), first_difference(got, plain, b.nq)
    assert plain.copies == 0 and got.copies == expected_copies(b) > 0
    # work done once: the collapsed batch does what the batch of first occurrences alone does
    alone = fresh(d, False)
    firsts = align(alone, sub_batch(b, first_occurrences(b)))
    alone.close()
    assert got.counters[:11] == firsts.counters[:11] and got.extra[:6] == firsts.extra[:6]
    assert got.counters[0] == b.nq - got.copies and plain.counters[0] == b.nq
    if extra3 is not None:
        assert got.extra[3] == extra3 and plain.extra[3] == extra3
    on.close(); off.close()
    return got


def test_collapsed_streams_equal_uncollapsed_and_oracle(ref, db):
    rng = np.random.default_rng(0xC0)
    distinct = mixed_distinct(ref, 14_000, 6_000, seed=0xC1)
    queries = duplicated(distinct, seed=0xC2) + near_copies(distinct, rng)
    order = rng.permutation(len(queries))
    queries = [queries[i] for i in order]
    pe_at = next(q for q in range(len(queries)) if len(queries[q][0]) == 2)
    b = batch_of(queries, shared=[pe_at, pe_at])  # two more queries on the very bytes of a pair: copies of it
    got = check_output_and_work(ref, db, b)
    assert got.copies >= b.nq - len(distinct) - 40 * 9
    oracle_sample_equal(ref, b, got, sorted(set(rng.choice(b.nq, 300, replace=False).tolist()) | {pe_at, b.nq - 2, b.nq - 1}))


def test_collapsed_long_reads(ref, db):
    """1 kb queries (mates over 320 bases: the gapped passes of long reads, with the rejection filter), several copies of a read per wave."""
    m1, m2 = synth.synthetic_paired_end(ref, 150, read_len=500, seed=0xC3)[:2]
    single = synth.synthetic_single_end(ref, 150, read_len=1000, seed=0xC4)[0]
    distinct = [([m1[i], m2[i]], 100.0, 50.0) for i in range(len(m1))] + [([r], 0.0, 1.0) for r in single]
    b = batch_of(duplicated(distinct, seed=0xC5, counts=(1, 3, 8, 20), p=(0.4, 0.3, 0.2, 0.1)))
    got = check_output_and_work(ref, db, b, extra3=1)
    oracle_sample_equal(ref, b, got, list(range(0, b.nq, max(1, b.nq // 60))))


def test_collapsed_wave_form(ref, db, monkeypatch):
    monkeypatch.setenv("XM_WAVE", "1")
    rng = np.random.default_rng(0xC6)
    distinct = mixed_distinct(ref, 1_500, 500, seed=0xC7)
    queries = duplicated(distinct, seed=0xC8) + near_copies(distinct, rng)
    b = batch_of([queries[i] for i in rng.permutation(len(queries))])
    on, off = fresh(db, True), fresh(db, False)
    got, plain = align(on, b), align(off, b)
    assert streams_equal(got, plain), first_difference(got, plain, b.nq)
    assert got.copies == expected_copies(b) > 0 and got.counters[0] + got.copies <= b.nq
    on.close(); off.close()


def test_collapse_edge_cases(ref, db):
    r = synth.synthetic_single_end(ref, 3, seed=0xC9)[0]
    on, off = fresh(db, True), fresh(db, False)
    one = batch_of([([r[0]], 0.0, 1.0)] * 100_000)
    got, plain = align(on, one), align(off, one)
    assert streams_equal(got, plain) and got.copies == 99_999 and got.counters[0] == 1 and plain.counters[0] == 100_000
    for b in (batch_of([([r[1]], 0.0, 1.0)]), batch_of([([r[k]], 0.0, 1.0) for k in range(3)]), batch_of(mixed_distinct(ref, 500, 200, seed=0xCA))):
        got, plain = align(on, b), align(off, b)
        assert streams_equal(got, plain) and got.copies == 0 and got.counters[0] == b.nq
    empty = batch_of([])
    assert len(align(on, empty)) == 0
    # a context on which collapsing was never enabled
    dup = batch_of(duplicated(mixed_distinct(ref, 300, 100, seed=0xCB), seed=0xCC))
    never = db.new_context()
    plain = align(never, dup)
    assert plain.copies == 0 and plain.counters[0] == dup.nq and streams_equal(plain, align(on, dup))
    on.close(); off.close(); never.close()


def test_collapse_over_successive_batches(ref, db):
    """Two batches with other duplicate patterns through stage / commit: nothing of the first survives in the second; then two contexts on one GPU."""
    a = batch_of(duplicated(mixed_distinct(ref, 3_000, 1_000, seed=0xCD), seed=0xCE))
    b = batch_of(duplicated(mixed_distinct(ref, 2_000, 500, seed=0xCF), seed=0xD0, counts=(1, 2), p=(0.5, 0.5)))
    arrays = [(x.mate_count, x.mate_offset, x.mate_length, x.codes, x.expected_inner, x.deviation) for x in (a, b, a, b)]
    off = fresh(db, False)
    want = list(off.align_stream(iter(arrays), PARAMS))
    on = fresh(db, True)
    got = list(on.align_stream(iter(arrays), PARAMS))
    for x, g, w in zip((a, b, a, b), got, want):
        assert streams_equal(g, w), first_difference(g, w, x.nq)
        assert g.copies == expected_copies(x) > 0 and w.copies == 0
    on.close(); off.close()
    two = multi.MultiGpuDatabase([("syn", ref)], [0, 0], collapse=True)
    got = list(two.align_stream(iter(arrays), PARAMS))
    for x, g, w in zip((a, b, a, b), got, want):
        assert streams_equal(g, w) and g.copies == expected_copies(x)
    two.close()


def test_pileup_after_collapsed_batch(ref, db):
    """xm_pileup_add_last reads the canonical streams: a collapsed batch piles up exactly as the uncollapsed one (depth, alternatives, middle depth, events)."""
    reads = synth.synthetic_single_end(ref, 3_000, seed=0xD1, indel_prob=0.3)[0]
    m1, m2 = synth.synthetic_paired_end(ref, 1_000, seed=0xD2, indel_prob=0.3)[:2]
    queries = duplicated([api.Query(x) for x in reads] + [api.Query(m1[i], m2[i], expected_inner_distance=100.0, spacing_deviation_per_unit_penalty=50.0) for i in range(len(m1))],
                         seed=0xD3)
    piles = []
    for collapse in (False, True):
        c = fresh(db, collapse)
        res = c.align_batch(queries, PARAMS)
        assert (res.copies > 0) == collapse
        m = pileup.MatchDatabase(c, 0.1)
        n_events = m.add_last(queries)
        depth, alt = m._sum(0)
        piles.append((n_events, depth, alt, m._middle(0), m._events(), m.mutations()))
        m.close(); c.close()
    (n0, d0, a0, mid0, e0, mu0), (n1, d1, a1, mid1, e1, mu1) = piles
    assert n0 == n1 > 100 and np.array_equal(d0, d1) and np.array_equal(a0, a1) and np.array_equal(mid0, mid1) and e0 == e1 and mu0 == mu1


def test_cli_collapse_identical_queries(ref, tmp_path):
    """python -m mapper_amd with and without --collapse-identical-queries: byte-identical outputs (streaming path and per-object path), one statistics line on stderr."""
    small = ref[:400_000]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(small) + "\n")
    reads = synth.synthetic_single_end(small, 1_500, seed=0xD4, indel_prob=0.3)[0]
    rng = np.random.default_rng(0xD5)
    picks = rng.choice(len(reads), 4_000)
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, k in enumerate(picks):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(reads[k]), "I" * len(reads[k])))
    env = dict(os.environ)
    env["PYTHONNOUSERSITE"] = "1"

    def run(tag, extra):
        outs = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("sam", "unaligned", "mutations", "refs")}
        argv = [sys.executable, "-m", "mapper_amd", "--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--out-sam", outs["sam"],
                "--out-unaligned", outs["unaligned"], "--batch-size", "1500"]
        if tag.startswith("obj"):
            argv += ["--out-mutations", outs["mutations"], "--snp-threshold", "0", "0", "--out-refs-map-count", outs["refs"]]
        r = subprocess.run(argv + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return {k: open(v, "rb").read() for k, v in outs.items() if os.path.exists(v)}, r

    for path in ("stream", "obj"):
        plain, rp = run(path + "0", [])
        got, rg = run(path + "1", ["--collapse-identical-queries"])
        assert plain == got and len(got["sam"]) > 100_000
        assert "Identical queries" not in rp.stderr
        line = [l for l in rg.stderr.splitlines() if l.startswith("Identical queries")]
        assert len(line) == 1 and int(line[0].split()[2]) > 1_000 and " of 4000 " in line[0], rg.stderr[-2000:]
        assert rp.stdout == rg.stdout
