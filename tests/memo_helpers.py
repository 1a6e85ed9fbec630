"""Shared helpers of tests/test_gpu_memo.py: batches with known duplicate structure, the key a query is remembered under, and what a context that has seen
some batches may serve of the next one - all computed here, in Python, from the queries' bytes."""
import numpy as np

import oracle_lib as o
from mapper_amd import api, synth

PARAMS = api.AlignmentParameters()


def batch_of(queries):
    """queries: list of (mates, expected_inner, deviation) -> QueryBatch."""
    return o.QueryBatch(queries)


def arrays_of(b):
    return b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation


def key_of(b, q):
    """What a query's alignment reads: mate count, mates (bytes, in order), the bit patterns of expected_inner and deviation."""
    mates = tuple(bytes(b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]]) for m in range(int(b.mate_count[q])))
    return (int(b.mate_count[q]), mates, np.float64(b.expected_inner[q]).view(np.int64).item(), np.float64(b.deviation[q]).view(np.int64).item())


def keys_of(b):
    return {key_of(b, q) for q in range(b.nq)}


def expected_copies(b):
    return b.nq - len(keys_of(b))


def first_occurrences(b):
    seen, firsts = set(), []
    for q in range(b.nq):
        k = key_of(b, q)
        if k not in seen:
            seen.add(k)
            firsts.append(q)
    return firsts


def expected_remembered(b, held):
    """b's representatives (first occurrences) whose key is in `held`, the keys of what the context aligned before."""
    return sum(1 for q in first_occurrences(b) if key_of(b, q) in held)


def sub_batch(b, idx):
    idx = list(idx)
    return o.QueryBatch([([b.codes[b.mate_offset[2 * q + m]:b.mate_offset[2 * q + m] + b.mate_length[2 * q + m]] for m in range(int(b.mate_count[q]))],
                          float(b.expected_inner[q]), float(b.deviation[q])) for q in idx])


def not_held(b, held):
    """b's first occurrences that `held` does not have: what a remembering context still aligns."""
    return [q for q in first_occurrences(b) if key_of(b, q) not in held]


def align(d, b, params=PARAMS):
    return d.align_arrays(*arrays_of(b), params)


def duplicated(distinct, seed, counts=(1, 2, 5), p=(0.6, 0.3, 0.1)):
    """every query of `distinct` a seeded random number of times, shuffled"""
    rng = np.random.default_rng(seed)
    reps = rng.choice(counts, size=len(distinct), p=p)
    out = [q for q, k in zip(distinct, reps) for _ in range(int(k))]
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def mixed_distinct(ref, n_se, n_pe, seed, read_len=150):
    se = synth.synthetic_single_end(ref, n_se, read_len=read_len, seed=seed)[0]
    m1, m2 = synth.synthetic_paired_end(ref, n_pe, read_len=read_len, seed=seed + 1)[:2]
    return [([r], 0.0, 1.0) for r in se] + [([m1[i], m2[i]], 100.0, 50.0) for i in range(n_pe)]


def near_copies(distinct, rng, n=40):
    """queries that differ from one of `distinct` in one thing each - one base changed, one base N, one base shorter, another expected_inner, mates swapped,
    another deviation, mate 1 alone: none of them may be served from it"""
    out = []
    se = [q for q in distinct if len(q[0]) == 1]
    pe = [q for q in distinct if len(q[0]) == 2]
    for k in range(n):
        (r,), e, d = se[int(rng.integers(len(se)))]
        i = int(rng.integers(len(r)))
        changed = r.copy(); changed[i] = {1: 2, 2: 4, 4: 8, 8: 1}.get(int(r[i]), 1)
        n_ = r.copy(); n_[i] = 15
        out += [([changed], e, d), ([n_], e, d), ([r[:-1].copy()], e, d), ([r], e + 1.0, d)]
        (a, b), e, d = pe[int(rng.integers(len(pe)))]
        out += [([b, a], e, d), ([a, b], e + 1.0, d), ([a, b], e, d * 2), ([a], 0.0, 1.0), ([a], e, d)]
    return out


def random_queries(n, length, seed):
    """uniformly random bases: on a synthetic reference of a megabase they align nowhere"""
    rng = np.random.default_rng(seed)
    return [([rng.choice(np.array([1, 2, 4, 8], dtype=np.uint8), size=length)], 0.0, 1.0) for _ in range(n)]


def unaligned_count(res):
    """queries whose result is one component without alignments"""
    return sum(1 for q in range(len(res)) if res.ints[res.int_off[q]] == 1 and res.ints[res.int_off[q] + 1] == 0)


def oracle_sample_equal(ref, b, got, idx):
    want = o.OracleReference([("syn", ref)]).align(sub_batch(b, idx), o.make_params())
    for k, q in enumerate(idx):
        gi = got.ints[got.int_off[q]:got.int_off[q + 1]]
        gd = np.asarray(got.dbls[got.dbl_off[q]:got.dbl_off[q + 1]]).view(np.int64)
        wi = want.ints[want.int_off[k]:want.int_off[k + 1]]
        wd = want.dbls[want.dbl_off[k]:want.dbl_off[k + 1]].view(np.int64)
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd), "query %d differs from the oracle" % q
