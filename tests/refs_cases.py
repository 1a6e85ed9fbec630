"""What the tests of the count per combination of contigs share (tests/test_refs_rules.py on the CPU, tests/test_gpu_refs_count.py on the GPU): recount(), the
count made here in Python - literally cli.ObjectSink's expression over the slices decoded by api.decode_streams: the yardstick for the C++ rules and the
kernels -, fold(), the host's half of the device count, and the cases the plan names.  The case file is summary_cases.write_streams'."""
import sam_cases as sc
import summary_cases as sm
from mapper_amd import api

NUM_CONTIGS = sm.NUM_CONTIGS
Malformed = sm.Malformed


def recount(arrays, num_contigs=NUM_CONTIGS):
    """{tuple of ascending contig indices: queries} over the aligned queries of the four streams, or Malformed(lowest malformed query) where the summary's
    recount says so (the walk and its conditions are the same)."""
    sm.recount(arrays, num_contigs=num_contigs)
    ints, dbls, io, do = arrays
    out = {}
    for q in range(len(io) - 1):
        comps = api.decode_streams(ints, dbls, io, do, q)
        if any(len(c) > 0 for c in comps):
            key = tuple(sorted({sa.contig for comp in comps for al in comp for sa in al.components}))
            out[key] = out.get(key, 0) + 1
    return out


def fold(records, leftovers):
    """records: (ids, count) per combination; leftovers: per left-over query the contigs of its sequence alignments -> the dict (set, sort, add one each)."""
    out = {}
    for ids, count in records:
        out[tuple(ids)] = out.get(tuple(ids), 0) + count
    for contigs in leftovers:
        key = tuple(sorted(set(contigs)))
        out[key] = out.get(key, 0) + 1
    return out


def on(contig, k=0, length=30):
    """One alignment of a single read on `contig`."""
    return (0.0, 0.5 + k, [(contig, k % 2, sc.whole(length, 100 * k))])


def random_streams(nq, seed=None):
    """nq queries of every kind, a fifth of them unaligned (none when nq == 1), on the four contigs of sam_cases."""
    return sc.random_case(1000 + nq if seed is None else seed, nq, read_len=None if nq < 1000 else 24, name_len=5, unaligned=0.2 if nq > 1 else 0.0)[1]


def same_combination_case(nq=4200):
    """Every aligned query on contigs {1, 3}; every fifth query unaligned."""
    s = sc.Streams()
    for q in range(nq):
        s.unaligned() if q % 5 == 4 else s.aligned([on(3, 0), on(1, 1)] if q % 2 else [on(1, 0), on(3, 1), on(1, 2)])
    return s


def own_combination_case(nq=4097, num_contigs=300):
    """Query q on {i, j}, no two queries on the same pair."""
    s, q = sc.Streams(), 0
    for i in range(num_contigs):
        for j in range(i + 1, num_contigs):
            if q == nq:
                return s
            s.aligned([on(j, 0), on(i, 1)])
            q += 1
    raise ValueError("not enough pairs")


def set_sizes_case():
    """Sets of exactly 8 (three queries, the contigs in three orders), of 9 (two queries) and of 40 distinct contigs (one), between queries on one contig."""
    s = sc.Streams()
    eight = list(range(10, 18))
    s.aligned([on(0)])
    s.aligned([on(c, k) for k, c in enumerate(eight)])
    s.aligned([on(c, k) for k, c in enumerate(reversed(eight))])
    s.aligned([on(c, k) for k, c in enumerate(range(9))])
    s.unaligned()
    s.aligned([on(c, k) for k, c in enumerate(eight[3:] + eight[:3] + eight)])  # (sixteen alignments, eight contigs)
    s.aligned([on(c, k) for k, c in enumerate(range(40))])
    s.aligned([on(c, k) for k, c in enumerate(reversed(range(9)))])
    s.aligned([on(0)])
    return s


def shapes_case():
    """One contig in three alignments of a query (a set of one); a pair on two contigs; a pair that fell back, its mates on two contigs; the same with one
    mate unaligned."""
    s = sc.Streams()
    s.aligned([on(2, 0, 70), on(2, 1, 70), on(2, 2, 70)])
    s.aligned([(0.4, 2.5, [(0, 0, sc.blocks_of(33, [("M", 10), ("I", 2), ("M", 20)], lead=1)), (1, 1, sc.blocks_of(27, [("M", 7), ("D", 2), ("M", 20)]))])])
    s.fallback([[(3.5, (0, 0, sc.whole(18, 40)))], [(12.25, (3, 1, sc.whole(19, 900))), (12.5, (0, 0, sc.whole(19, 10)))]])
    s.fallback([[], [(12.25, (3, 1, sc.whole(19, 900)))]])
    s.fallback([[], []])
    return s


def wide_between_unaligned_case(nq, at, n=40):
    """nq single reads, all unaligned but query `at`, which has n alignments on n contigs."""
    s = sc.Streams()
    for q in range(nq):
        s.aligned([on(k, k) for k in range(n)]) if q == at else s.unaligned()
    return s
