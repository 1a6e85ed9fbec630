"""Shared helpers of the test-suite."""
import json
import os
import numpy as np

import oracle_lib
from mapper_amd import api, sam, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_reference.json")))


def streams_equal(a, b):
    """bit-exact equality of two result streams (ints, doubles compared by bit pattern, offsets)."""
    return (np.array_equal(a.int_off, b.int_off) and np.array_equal(a.dbl_off, b.dbl_off) and np.array_equal(a.ints, b.ints)
            and np.array_equal(np.asarray(a.dbls).view(np.int64), np.asarray(b.dbls).view(np.int64)))


def first_difference(a, b, n):
    for q in range(n):
        x = api.decode_streams(a.ints, a.dbls, a.int_off, a.dbl_off, q)
        y = api.decode_streams(b.ints, b.dbls, b.int_off, b.dbl_off, q)
        fx = [[(al.penalty, [(s.contig, s.reference_reversed, [(k.startA, k.startB, k.lengthA, k.lengthB) for k in s.sections]) for s in al.components]) for al in c] for c in x]
        fy = [[(al.penalty, [(s.contig, s.reference_reversed, [(k.startA, k.startB, k.lengthA, k.lengthB) for k in s.sections]) for s in al.components]) for al in c] for c in y]
        if fx != fy:
            return "query %d: %r != %r" % (q, fx, fy)
    return None


def se_batch(reads):
    nq, L = reads.shape
    mc = np.ones(nq, np.int32)
    mo = np.zeros(2 * nq, np.int64); mo[0::2] = np.arange(nq, dtype=np.int64) * L
    ml = np.zeros(2 * nq, np.int32); ml[0::2] = L
    return oracle_lib.QueryBatch.from_arrays(mc, mo, ml, np.ascontiguousarray(reads.reshape(-1)), np.zeros(nq), np.ones(nq))


def ragged_se_batch(reads):
    """single reads of different lengths (a list of code arrays)"""
    nq = len(reads)
    lens = np.array([len(r) for r in reads], np.int64)
    mc = np.ones(nq, np.int32)
    mo = np.zeros(2 * nq, np.int64); mo[0::2] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ml = np.zeros(2 * nq, np.int32); ml[0::2] = lens
    return oracle_lib.QueryBatch.from_arrays(mc, mo, ml, np.ascontiguousarray(np.concatenate(reads)), np.zeros(nq), np.ones(nq))


def pe_batch(m1, m2, expected=100.0, dev=50.0):
    nq, L = m1.shape
    codes = np.ascontiguousarray(np.concatenate([m1, m2], axis=1).reshape(-1))
    mc = np.full(nq, 2, np.int32)
    mo = np.zeros(2 * nq, np.int64); mo[0::2] = np.arange(nq, dtype=np.int64) * 2 * L; mo[1::2] = mo[0::2] + L
    ml = np.full(2 * nq, L, np.int32)
    return oracle_lib.QueryBatch.from_arrays(mc, mo, ml, codes, np.full(nq, expected), np.full(nq, dev))


def _gather_slices(data, starts, lens):
    """data[starts[i] : starts[i] + lens[i]] for every i, concatenated -> (array, offsets of the pieces in it: len(starts) + 1 of them, by np.cumsum)."""
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    take = np.repeat(starts - off[:-1], lens) + np.arange(off[-1], dtype=np.int64)
    return np.ascontiguousarray(np.asarray(data)[take]), off


def compose_batch(U, idx):
    """The batch whose query j is query idx[j] of the oracle_lib.QueryBatch U (its mates, expected inner distance and deviation): the bases are copied,
    every query of the result has bases of its own."""
    idx = np.asarray(idx, np.int64)
    ml = np.ascontiguousarray(U.mate_length.reshape(-1, 2)[idx].reshape(-1))
    codes, off = _gather_slices(U.codes, U.mate_offset.reshape(-1, 2)[idx].reshape(-1), ml)
    mo = np.where(ml > 0, off[:-1], 0)
    if len(codes) == 0:
        codes = np.zeros(1, np.uint8)
    return oracle_lib.QueryBatch.from_arrays(U.mate_count[idx].copy(), np.ascontiguousarray(mo), ml, codes, U.expected_inner[idx].copy(), U.deviation[idx].copy())


def alignments_per_query(s):
    """The number of alignments in every query's slice of the streams s (the sum over its components)."""
    out = np.zeros(len(s.int_off) - 1, np.int64)
    for q in range(len(out)):
        out[q] = sum(len(als) for als in s.query(q))
    return out


def align_each(R, U, params, threads=1):
    """The oracle's streams of the batch U (one call of R.align) with what compose_streams needs beside them: .per_query, an int64 array [U.nq, 24] of every
    query's own contribution to the oracle's counters - the oracle reports counters per call, so each query is aligned again in a batch of its own - and
    .alignments, the alignments in every query's slice.  A query's result does not depend on its batch: the one-query calls must return the slices of the
    call over U and their counters must add up to its counters, which is asserted here."""
    want = R.align(U, params, threads=threads)
    want.alignments = alignments_per_query(want)
    want.per_query = np.zeros((U.nq, 24), np.int64)
    for q in range(U.nq):
        one = R.align(compose_batch(U, [q]), params, threads=1)
        assert np.array_equal(one.ints, want.ints[want.int_off[q]:want.int_off[q + 1]]), ("a query's result depends on its batch", q)
        want.per_query[q] = one.counters
    assert want.per_query.sum(axis=0).tolist() == [int(x) for x in want.counters], (want.per_query.sum(axis=0).tolist(), want.counters)
    return want


def compose_streams(want_U, idx):
    """What a batch of the queries idx of U (compose_batch) must give, from the oracle's run over U (align_each), in plain numpy: every query's int and
    double slices in batch order, the offsets by np.cumsum, .counters = the sum of the queries' own contributions to the oracle's counters and
    .alignments_out = the alignments in the slices."""
    idx = np.asarray(idx, np.int64)
    ints, int_off = _gather_slices(want_U.ints, want_U.int_off[idx], want_U.int_off[idx + 1] - want_U.int_off[idx])
    dbls, dbl_off = _gather_slices(want_U.dbls, want_U.dbl_off[idx], want_U.dbl_off[idx + 1] - want_U.dbl_off[idx])
    s = oracle_lib.Streams(ints, dbls, int_off, dbl_off, [int(x) for x in want_U.per_query[idx].sum(axis=0)])
    s.alignments_out = int(want_U.alignments[idx].sum())
    return s


def check_align_case(case, comps, ref_codes):
    """Checks the expectations a reference JUnit case pins on the decoded QueryAlignments (list of components)."""
    e = case["expect"]
    top = comps[0] if len(comps) == 1 else []
    assert len(top) == e["num"], "%s: expected %d alignments, got %d" % (case["name"], e["num"], len(top))
    if "alignedB0" in e:
        s = top[0].components[0]
        q = api.encode(case["mates"][0])
        if s.reference_reversed:
            q = api.reverse_complement(q)
        assert s.aligned_text(q, ref_codes)[1] == e["alignedB0"], case["name"]
    if "startsB" in e:
        got = sorted([s.start_index_b() for s in al.components] for al in top)
        # the order of equal-penalty alignments comes from a HashSet in the reference (QueryMatch_Aligner.java:86-92): compared as a set
        assert got == sorted(e["startsB"]), case["name"]


def sam_text(query, comps, names):
    return "".join(line + "\n" for line in sam.records(query, comps, names))


def sprinkle_ambiguity(reads, seed=3):
    """Copies of `reads` (code arrays [n, L]) with 0-3 IUPAC ambiguity codes each (N, R, Y, M, K, V, B) and, in every 50th read, a run of 2-11 N's."""
    rng = np.random.default_rng(seed)
    out = reads.copy()
    codes = np.array([15, 15, 15, 5, 10, 3, 12, 7, 14], np.uint8)
    for q in range(len(out)):
        k = rng.integers(0, 4)
        pos = rng.integers(0, out.shape[1], size=k)
        out[q, pos] = codes[rng.integers(0, len(codes), size=k)]
        if q % 50 == 0:
            p0 = rng.integers(0, out.shape[1] - 12)
            out[q, p0:p0 + rng.integers(2, 12)] = 15
    return out


def ambiguous_reference(n, seed, n_runs=6, n_codes=40):
    """A synthetic reference (code array) with runs of N (1-40 long) and scattered IUPAC codes."""
    from mapper_amd import synth
    ref = synth.synthetic_reference(n, seed=seed).copy()
    rng = np.random.default_rng(seed)
    for _ in range(n_runs):
        p0 = int(rng.integers(0, n - 50))
        ref[p0:p0 + int(rng.integers(1, 41))] = 15
    codes = np.array([15, 5, 10, 3, 12, 6, 9, 7, 11, 13, 14], np.uint8)
    ref[rng.integers(0, n, size=n_codes)] = codes[rng.integers(0, len(codes), size=n_codes)]
    return ref


IUPAC_2WAY = np.array([3, 5, 9, 6, 10, 12], np.uint8)   # M R W S Y K
IUPAC_3WAY = np.array([7, 11, 13, 14], np.uint8)        # V H D B


def heavy_ambiguity(reads, seed=11):
    """Copies of `reads` (code arrays [n, L]) in which read q carries ambiguity of class q mod 16: a fraction of its positions - 1 %, 10 %, 50 %, 90 %, 100 % -
    replaced by N (classes 0-4), by two-way IUPAC codes (5-9) or by three-way codes (10-12: 10 %, 50 %, 100 %); 13: a run of N at the read's start of a
    third to all of its length; 14: the same at its end; 15: untouched.  What real FASTQ holds (all-N reads, N tails) and what no other test reaches: the
    reference bounds the combinations per block, not the ambiguous bases per read (HashBlock_ParentRow.java:10,109,165)."""
    rng = np.random.default_rng(seed)
    out = reads.copy()
    n, L = out.shape
    fr = [0.01, 0.1, 0.5, 0.9, 1.0]
    for q in range(n):
        c = q % 16
        if c < 5:
            out[q, rng.random(L) < fr[c]] = 15
        elif c < 10:
            m = rng.random(L) < fr[c - 5]
            out[q, m] = IUPAC_2WAY[rng.integers(0, len(IUPAC_2WAY), int(m.sum()))]
        elif c < 13:
            m = rng.random(L) < [0.1, 0.5, 1.0][c - 10]
            out[q, m] = IUPAC_3WAY[rng.integers(0, len(IUPAC_3WAY), int(m.sum()))]
        elif c == 13:
            out[q, :int(rng.integers(L // 3, L + 1))] = 15
        elif c == 14:
            out[q, L - int(rng.integers(L // 3, L + 1)):] = 15
    return out


def low_complexity_reads(n, L, seed=12):
    """homopolymer, dinucleotide and short-period reads (code arrays [n, L]), a few with one ambiguity code in them"""
    rng = np.random.default_rng(seed)
    acgt = np.array([1, 2, 4, 8], np.uint8)
    out = np.zeros((n, L), np.uint8)
    for q in range(n):
        period = [1, 2, 3, 5][q % 4]
        unit = acgt[rng.integers(0, 4, period)]
        out[q] = np.tile(unit, L // period + 1)[:L]
        if q % 5 == 4:
            out[q, int(rng.integers(0, L))] = [15, 5, 14][q % 3]
    return out


def bound_problems(seed, count):
    """Random problems for the rejection filter in front of PathAligner (mapper_amd/csrc/xm_bound.h) and the oracle's observer of it: tuples
    (params dict, query codes, query_rc, start_a, end_a, reference codes, start_b, end_b, predicted_best_offset).  A query section is a window of the reference
    put through one of several error regimes (none ... unrelated text), so that searches that align, searches that fail narrowly and searches that fail by far
    all occur; windows shorter than the query, windows at the ends of the reference, long windows, wide bands, ambiguity codes and price sets that are not
    multiples of the filter's grid are mixed in."""
    rng = np.random.default_rng(seed)
    acgt = np.array([1, 2, 4, 8], dtype=np.uint8)
    comp = np.zeros(16, dtype=np.uint8)
    for c in range(16):
        comp[c] = ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3)
    out = []
    for _ in range(count):
        n = int(rng.choice([10, 25, 40, 60, 91, 91, 91, 120, 182, 250, 400]))
        slack_lo, slack_hi = (int(x) for x in rng.choice([0, 0, 3, 10, 25, 60, 140], 2))
        if rng.random() < 0.08:
            slack_lo, slack_hi = int(rng.integers(100, 300)), int(rng.integers(100, 300))   # a window far longer than the query
        R = int(rng.integers(n + slack_lo + slack_hi + 40, n + slack_lo + slack_hi + 400))
        ref = acgt[rng.integers(0, 4, R)]
        where = rng.random()
        if where < 0.08:
            start_b = 0
        elif where < 0.16:
            start_b = R - (n + slack_lo + slack_hi)
        else:
            start_b = int(rng.integers(1, R - (n + slack_lo + slack_hi)))
        end_b = start_b + slack_lo + n + slack_hi
        # the query section: the window's middle, mutated
        regime = rng.choice(["none", "subs", "indel", "mixed", "heavy", "unrelated"], p=[0.08, 0.17, 0.2, 0.25, 0.2, 0.1])
        src = ref[start_b + slack_lo: start_b + slack_lo + n + 40 if start_b + slack_lo + n + 40 <= R else R].copy()
        sub, ind = {"none": (0, 0), "subs": (0.04, 0), "indel": (0.005, 0.01), "mixed": (0.03, 0.02), "heavy": (0.06, 0.05), "unrelated": (0, 0)}[regime]
        seq = []
        i = 0
        while len(seq) < n and i < len(src):
            u = rng.random()
            if u < ind / 2:
                seq.extend(acgt[rng.integers(0, 4, int(rng.integers(1, 4)))])   # insertion
            elif u < ind:
                i += int(rng.integers(1, 4))                                      # deletion
                continue
            b = src[i]
            if rng.random() < sub:
                b = acgt[(int(np.log2(b)) + int(rng.integers(1, 4))) & 3]
            seq.append(b)
            i += 1
        sec = np.array(seq[:n], dtype=np.uint8)
        if regime == "unrelated" or len(sec) < n:
            sec = acgt[rng.integers(0, 4, n)]
        if rng.random() < 0.1:   # ambiguity codes in the query or the window
            k = int(rng.integers(1, 6))
            sec[rng.integers(0, n, k)] = rng.choice([15, 5, 10, 3, 12, 7, 14], k)
            ref[rng.integers(start_b, end_b, k)] = rng.choice([15, 5, 10, 6, 9, 11, 13], k)
        if rng.random() < 0.07:  # a window shorter than the query
            end_b = start_b + max(1, n - int(rng.integers(1, 30)))
        # the section inside a longer query, possibly of its reverse complement
        pre, post = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        view = np.concatenate([acgt[rng.integers(0, 4, pre)], sec, acgt[rng.integers(0, 4, post)]])
        query_rc = bool(rng.random() < 0.5)
        query = comp[view[::-1]] if query_rc else view   # the stored query; the view the aligner sees is `view`
        start_a, end_a = pre, pre + n
        offset = (start_b + slack_lo) - start_a + int(rng.choice([0, 0, 0, 1, -2, 7]))
        prm = {}
        u = rng.random()
        if u < 0.25:
            prm = dict(MutationPenalty=float(rng.choice([1.0, 0.8, 1.37, 2.0])), InsertionStart_Penalty=float(rng.choice([1.5, 0.9, 2.25, 0.41])),
                       InsertionExtension_Penalty=float(rng.choice([0.6, 0.3, 0.77, 1.0])), DeletionStart_Penalty=float(rng.choice([1.5, 1.0, 3.1])),
                       DeletionExtension_Penalty=float(rng.choice([0.5, 0.25, 0.61])), AmbiguityPenalty=float(rng.choice([0.1, 0.0, 0.33])))
        prm["MaxErrorRate"] = float(rng.choice([0.1, 0.1, 0.1, 0.1091, 0.05, 0.02, 0.2, 0.3, 0.0]))
        out.append((prm, query, query_rc, start_a, end_a, ref, start_b, end_b, offset))
    return out


def filter_counters(device_counters, device_extra, oracle_counters):
    """The work counters of a call that ran with the rejection filter (mapper_amd/csrc/xm_bound.h) against the oracle's with its observer on (oracle_lib.observe_bound):
    -> (equal, what).  The product skips the searches the filter proves null (their nodes) and the whole chain of the pieces it proves unalignable (their PathAligner calls and
    nodes); the observer counts both, and what the search-level filter sees outside rejected pieces."""
    oc = [int(x) for x in oracle_counters]
    calls, nodes, rejects, reject_nodes, checks, piece_checks, piece_rejects, skipped_calls, skipped_nodes = oc[6], oc[7], oc[11], oc[12], oc[13], oc[14], oc[15], oc[16], oc[17]
    want = dict(searches_examined=checks, searches_rejected=rejects, pieces_examined=piece_checks, pieces_rejected=piece_rejects, path_aligner_calls=calls - skipped_calls,
                nodes=nodes - reject_nodes - skipped_nodes)
    got = dict(searches_examined=int(device_extra[0]), searches_rejected=int(device_extra[1]), pieces_examined=int(device_extra[4]), pieces_rejected=int(device_extra[5]),
               path_aligner_calls=int(device_counters[5]), nodes=int(device_counters[6]))
    return got == want, dict(device=got, oracle_observer=want, reference=dict(path_aligner_calls=calls, nodes=nodes, searches_returning_null=oc[9], nodes_in_null_searches=oc[10],
                                                                                nodes_in_rejected_searches=reject_nodes, calls_in_rejected_pieces=skipped_calls, nodes_in_rejected_pieces=skipped_nodes))


def long_read_batch(ref, n_reads, sub, indel, seed=0x5EED0004, starts=None):
    """BASELINE.json configs[4]'s queries: 10 kb reads (synth.synthetic_long_reads: per base a substitution with probability `sub`, an indel event with
    probability `indel`), either strand, cut into 1 kb sections as the CLI cuts them (cli.split_sections).  `starts`: template starts in `ref` (default: uniform)."""
    from mapper_amd import cli
    if starts is None:
        starts = (synth.splitmix64(seed, n_reads) % np.uint64(len(ref) - 12_600)).astype(np.int64)
    strand = (synth.splitmix64(seed ^ 0x57A, n_reads) >> np.uint64(63)).astype(np.uint8)
    reads = synth.synthetic_long_reads(ref, starts, 10_000, seed=seed, sub_rate=sub, indel_rate=indel, strand=strand)
    return oracle_lib.QueryBatch([([r[a_:b_].copy()], 0.0, 1.0) for r in reads for a_, b_ in cli.split_sections(10_000, 1000)])


def _cpu_filter_fuzz():
    """scripts/cpu_filter_fuzz.py as a module (its batch generator is shared with the GPU tier; the script stays runnable on its own)."""
    global _FILTER_FUZZ
    if _FILTER_FUZZ is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location("cpu_filter_fuzz", os.path.join(ROOT, "scripts", "cpu_filter_fuzz.py"))
        _FILTER_FUZZ = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_FILTER_FUZZ)
    return _FILTER_FUZZ


_FILTER_FUZZ = None


def filter_fuzz_reads(rng, ref, n):
    """scripts/cpu_filter_fuzz.py filter_fuzz_reads: n reads of lengths 330-1500 in five error regimes, N bases in some (an oracle_lib.QueryBatch)."""
    return _cpu_filter_fuzz().filter_fuzz_reads(rng, ref, n)


def filter_fuzz_case(rng, n_lo, n_hi):
    """scripts/cpu_filter_fuzz.py filter_fuzz_case: -> (reference codes, params dict, batch of n_lo .. n_hi - 1 reads)."""
    return _cpu_filter_fuzz().filter_fuzz_case(rng, n_lo, n_hi)


# the filter's grid and limits (mapper_amd/csrc/xm_bound.h): the edge table below is built from them
BOUND_SCALE, BOUND_KMAX, BOUND_MMAX, BOUND_KMAX_WIDE, BOUND_MMAX_WIDE = 60, 200, 456, 2048, 4096
_DEFAULT_PRICES = dict(MutationPenalty=1.0, InsertionStart_Penalty=1.5, InsertionExtension_Penalty=0.6, DeletionStart_Penalty=1.5, DeletionExtension_Penalty=0.5,
                       MaxErrorRate=0.1, AmbiguityPenalty=0.1)


def bound_grid(prm, n):
    """boundPrices + boundBand of xm_bound.h restated for prices the filter takes (a search problem, not a piece): -> (thr, maxIns, maxDel) on the 1/60 grid."""
    import math
    p = dict(_DEFAULT_PRICES, **prm)
    s = float(BOUND_SCALE)
    t = math.floor((n * p["MaxErrorRate"] + 0.000001 + 0.0000001) * s)
    isie, ie = math.floor((p["InsertionStart_Penalty"] + p["InsertionExtension_Penalty"]) * s), math.floor(p["InsertionExtension_Penalty"] * s)
    dsde, de = math.floor((p["DeletionStart_Penalty"] + p["DeletionExtension_Penalty"]) * s), math.floor(p["DeletionExtension_Penalty"] * s)
    max_ins = 0 if t < isie else (t - isie) // ie + 1
    max_del = 0 if t < dsde else (t - dsde) // de + 1
    return t, max_ins, max_del


def band_slots(prm, n, m):
    """K of boundBand: the band slots a search of an n-base section over an m-base window needs (m >= n or m < n)."""
    _, max_ins, max_del = bound_grid(prm, n)
    d0, d1 = (0, m - n) if m >= n else (-(n - m), 0)
    return min(d1 + max_del, m) - max(d0 - max_ins, -n) + 1


def window_for_slots(prm, n, k):
    """The window length m >= n at which a search of an n-base section needs exactly k band slots (no clamp at either edge of the band)."""
    _, max_ins, max_del = bound_grid(prm, n)
    m = k - 1 - max_ins - max_del + n
    assert m >= n and max_ins <= n and max_del <= m - n + max_del <= m and band_slots(prm, n, m) == k, (prm, n, k, m)
    return m


def bound_edge_problems():
    """A deterministic table of problems for the rejection filter (mapper_amd/csrc/xm_bound.h) that land exactly on the limits where it changes form or declines:
    tuples (name, params dict, query codes, query_rc, start_a, end_a, reference codes, start_b, end_b, predicted_best_offset), as bound_problems.
    The band sizes come from boundBand's own formulas (band_slots / window_for_slots).  Query sections are the window's middle with errors placed where
    chooseSearchReverse (PathAligner.java:17-53) should send the search - errors in the first part of the section: forward; in the last part: reverse."""
    rng = np.random.default_rng(0xED6E)
    acgt = np.array([1, 2, 4, 8], dtype=np.uint8)
    comp = np.zeros(16, dtype=np.uint8)
    for c in range(16):
        comp[c] = ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3)
    out = []

    def sub(b):
        return acgt[(int(np.log2(b)) + int(rng.integers(1, 4))) & 3]

    def problem(name, prm, n, m, errors=0, where="first", at_start=False, at_end=False, inset=0, query_rc=False, indels=0, section=None, ambiguity=0):
        """n-base section against an m-base window; the section is window[lo : lo + n] (m >= n: centred; m < n: the window plus n - m bases beside it).
        errors substitutions in the first / last third of the section (`where`: "first" -> forward search, "last" -> reverse, "all": spread); indels deletions
        of single bases spread over the section; `section`: "unrelated" for random text (a search that fails by far)."""
        pad = 30
        R = m + 2 * pad + max(0, n - m) + 20
        ref = acgt[rng.integers(0, 4, R)]
        start_b = inset if at_start else (R - m - inset if at_end else pad)
        end_b = start_b + m
        lo = start_b + (m - n) // 2 if m >= n else start_b
        src = ref[lo: lo + n + indels].copy()
        if indels:
            drop = np.linspace(n // 10, n + indels - n // 10, indels).astype(int)
            src = np.delete(src, drop)
        sec = src[:n].copy()
        if errors:
            third = max(1, n // 3)
            pos = {"first": rng.choice(third, min(errors, third), replace=False), "last": n - 1 - rng.choice(third, min(errors, third), replace=False),
                   "all": rng.choice(n, errors, replace=False)}[where]
            for i in pos:
                sec[i] = sub(sec[i])
        if section == "unrelated":
            sec = acgt[rng.integers(0, 4, n)]
        if ambiguity:
            sec[rng.integers(0, n, ambiguity)] = rng.choice([15, 5, 10, 3, 12, 7, 14], ambiguity)
            ref[rng.integers(start_b, end_b, ambiguity)] = rng.choice([15, 5, 10, 6, 9, 11, 13], ambiguity)
        pre, post = 7, 5
        view = np.concatenate([acgt[rng.integers(0, 4, pre)], sec, acgt[rng.integers(0, 4, post)]])
        query = comp[view[::-1]] if query_rc else view
        offset = lo - pre
        out.append((name, dict(prm), query, query_rc, pre, pre + n, ref, start_b, end_b, offset))

    d = {}
    # LDS region <-> wide band in HBM: K = 200 / 201 slots (m <= 456), m = 456 / 457 bases (K <= 200)
    for k in (BOUND_KMAX, BOUND_KMAX + 1):
        m = window_for_slots(d, 100, k)
        problem("K=%d aligns" % k, d, 100, m, errors=4, where="all")
        problem("K=%d fails" % k, d, 100, m, errors=14, where="all", query_rc=True)
    for m in (BOUND_MMAX, BOUND_MMAX + 1):
        assert band_slots(d, 420, m) <= BOUND_KMAX
        problem("m=%d aligns" % m, d, 420, m, errors=20, where="all")
        problem("m=%d fails" % m, d, 420, m, errors=35, where="all", indels=8, query_rc=True)
    # taken <-> declined: K = 2048 / 2049 slots (m <= 4096), m = 4096 / 4097 bases (K <= 2048)
    for k in (BOUND_KMAX_WIDE, BOUND_KMAX_WIDE + 1):
        m = window_for_slots(d, 100, k)
        problem("K=%d aligns" % k, d, 100, m, errors=3, where="all")
        problem("K=%d fails" % k, d, 100, m, section="unrelated")
    for m in (BOUND_MMAX_WIDE, BOUND_MMAX_WIDE + 1):
        assert band_slots(d, 4000, m) <= BOUND_KMAX_WIDE
        problem("m=%d aligns" % m, d, 4000, m, errors=40, where="all", query_rc=True)
    # a window shorter than the query (the foot branch): by 1, 2 and n - 1 bases
    for short in (1, 2, 59):
        problem("foot -%d aligns" % short, d, 60, 60 - short, errors=1, where="all")
        problem("foot -%d fails" % short, d, 60, 60 - short, section="unrelated", query_rc=True)
    # windows at either end of the contig and one base in from it, both search directions, both strands
    for where in ("first", "last"):
        for end in ("start", "end"):
            for inset in (0, 1):
                for rc in (False, True):
                    problem("%s of contig +%d, errors %s, rc %d" % (end, inset, where, rc), d, 90, 100, errors=5, where=where,
                            at_start=end == "start", at_end=end == "end", inset=inset, query_rc=rc)
                problem("%s of contig +%d, errors %s, fails" % (end, inset, where), d, 90, 100, errors=14, where=where, at_start=end == "start", at_end=end == "end", inset=inset)
    # the budget: just below and at the 60 000-unit cap (n = m = 1000: the band clamps at both edges, K = n + m + 1), on an exact grid multiple, and just
    # below one by less than / more than the 1e-6 + 1e-7 the rounding adds (a section whose best path costs exactly 10: ten mismatches at 1.0)
    problem("budget 59999 units", dict(MaxErrorRate=59999.5 / 60 / 1000), 1000, 1000, errors=30, where="all")
    problem("budget 60000 units", dict(MaxErrorRate=1.0), 1000, 1000, errors=30, where="all")
    for rate in (0.1, 0.1 - 5e-9, 0.1 - 2e-8, 0.1 + 5e-9):
        problem("budget %r x 100, best path 10" % rate, dict(MaxErrorRate=rate), 100, 100, errors=10, where="all")
    problem("budget 9 exactly, best path 9", dict(MaxErrorRate=0.1), 90, 90, errors=9, where="all")
    # prices at the grid's limits
    problem("extension 1/60", dict(InsertionExtension_Penalty=1 / 60, DeletionExtension_Penalty=1 / 60), 40, 60, errors=3, where="all")
    problem("extension 1/60 fails", dict(InsertionExtension_Penalty=1 / 60, DeletionExtension_Penalty=1 / 60), 40, 60, section="unrelated")
    problem("insertion extension below 1/60", dict(InsertionExtension_Penalty=np.nextafter(1 / 60, 0)), 40, 60, errors=3, where="all")
    problem("deletion extension below 1/60", dict(DeletionExtension_Penalty=np.nextafter(1 / 60, 0)), 40, 60, errors=3, where="all")
    problem("start penalties 0", dict(InsertionStart_Penalty=0.0, DeletionStart_Penalty=0.0), 80, 90, errors=6, indels=3, where="all")
    problem("start penalties 0 fails", dict(InsertionStart_Penalty=0.0, DeletionStart_Penalty=0.0), 80, 90, section="unrelated")
    problem("mutation 0", dict(MutationPenalty=0.0), 80, 90, errors=20, where="all")
    problem("mutation 0, indels", dict(MutationPenalty=0.0), 80, 90, indels=12, where="all")
    for amb in (500.0, 500.02):
        problem("ambiguity %r" % amb, dict(AmbiguityPenalty=amb), 80, 90, errors=2, where="all", ambiguity=3)
    problem("ambiguity 0 with codes", dict(AmbiguityPenalty=0.0), 80, 90, errors=4, where="all", ambiguity=6)
    problem("ambiguity codes, defaults", d, 120, 130, errors=6, where="last", ambiguity=5, query_rc=True)
    # prices the CLI would refuse but the C ABI takes (xm_params): non-finite, out of range, a negative start with a large extension
    inf, nan = float("inf"), float("nan")
    for key in ("MutationPenalty", "InsertionStart_Penalty", "InsertionExtension_Penalty", "DeletionStart_Penalty", "DeletionExtension_Penalty", "AmbiguityPenalty"):
        for v in (nan, inf, -inf, 1e12, -1e12):
            problem("%s=%r" % (key, v), {key: v}, 40, 50, errors=3, where="all")
    problem("MaxErrorRate=nan", dict(MaxErrorRate=nan), 40, 50, errors=3, where="all")
    problem("MaxErrorRate=inf", dict(MaxErrorRate=inf), 40, 50, errors=3, where="all")
    problem("insertion start -1e12, extension 1e12", dict(InsertionStart_Penalty=-1e12, InsertionExtension_Penalty=1e12 + 0.6), 40, 50, errors=3, where="all")
    problem("deletion start -1e12, extension 1e12", dict(DeletionStart_Penalty=-1e12, DeletionExtension_Penalty=1e12 + 0.5), 40, 50, errors=3, where="all")
    problem("insertion start -666, extension 666.67", dict(InsertionStart_Penalty=-666.0, InsertionExtension_Penalty=666.67), 40, 50, errors=3, where="all")
    problem("deletion start -500, extension 500.5", dict(DeletionStart_Penalty=-500.0, DeletionExtension_Penalty=500.5), 40, 50, section="unrelated")
    return out


# rows of bound_edge_problems whose outcome is part of what the table is for: True = the filter must take the problem, False = it must decline it
BOUND_EDGE_TAKEN = {"K=200 aligns": True, "K=201 aligns": True, "m=456 aligns": True, "m=457 aligns": True, "K=2048 aligns": True, "K=2048 fails": True,
                    "K=2049 aligns": False, "K=2049 fails": False, "m=4096 aligns": True, "m=4097 aligns": False, "foot -59 aligns": True,
                    "start of contig +0, errors first, rc 0": True, "start of contig +0, errors last, rc 0": False, "end of contig +0, errors first, rc 0": False,
                    "end of contig +0, errors last, rc 0": True, "start of contig +1, errors last, rc 1": True, "end of contig +1, errors first, rc 1": True,
                    "budget 59999 units": True, "budget 60000 units": False, "extension 1/60": True, "insertion extension below 1/60": False,
                    "deletion extension below 1/60": False, "start penalties 0": True, "mutation 0": True, "ambiguity 500.0": True, "ambiguity 500.02": False,
                    "insertion start -666, extension 666.67": False, "deletion start -500, extension 500.5": False}


def bound_edge_search_runs(prm):
    """False for the rows of bound_edge_problems whose prices the reference's search has no meaning for (NaN, infinities, |price| >= 1e6): there only the
    observer's prices are compared (oracle_lib.kat_bound_prices), not a search."""
    return all(np.isfinite(v) and abs(v) < 1e6 for v in prm.values())


def check_bound_edges(run_filter):
    """Every problem of bound_edge_problems through run_filter(params dict, query, query_rc, start_a, end_a, reference, start_b, end_b, offset) -> (taken, rejected, cells)
    against the oracle's observer of the same bound: the same verdict (declined / taken / rejected), nothing rejected that the reference's search found, cells <= n x m
    (none when declined); the rows of BOUND_EDGE_TAKEN land on the side of the limit they were built for.  Rows with prices the search has no meaning for: the observer
    declines them, and so must the filter.  -> {name: (verdict, found)} (verdict -1: prices only)."""
    seen = {}
    for name, prm, q, rc, sa, ea, ref, sb, eb, off in bound_edge_problems():
        taken, rejected, cells = run_filter(prm, q, rc, sa, ea, ref, sb, eb, off)
        p = oracle_lib.make_params(prm)
        if bound_edge_search_runs(prm):
            verdict, found, _ = oracle_lib.kat_bound(p, q, rc, sa, ea, ref, sb, eb, off)   # (raises if the observer's bound rejected a search that aligned)
        else:
            verdict, found = -1, 0
            assert oracle_lib.kat_bound_prices(p, (ea - sa) * p.MaxErrorRate) is None, name
        want = (1 if verdict > 0 else 0, 1 if verdict == 2 else 0)
        assert (taken, rejected) == want, (name, "filter (taken, rejected)", (taken, rejected), "observer", want, "found", found)
        assert not (rejected and found), name
        assert cells <= (ea - sa) * (eb - sb) if taken else cells == 0, (name, cells)
        if name in BOUND_EDGE_TAKEN:
            assert bool(taken) == BOUND_EDGE_TAKEN[name], (name, taken)
        seen[name] = (verdict, found)
    return seen
