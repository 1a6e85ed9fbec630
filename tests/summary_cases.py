"""What the tests of the batch summary share (tests/test_summary_rules.py on the CPU, tests/test_gpu_summary.py on the GPU): recount(), the summary of result
streams counted here in Python from nothing but the stream layout of include/xmapper_hip.h:73-82 - the yardstick for the C++ rules and the kernels -, the
case file tests/summary_rules_main.cpp reads, and cases the SAM tests do not have."""
import struct

import numpy as np

import sam_cases as sc

NUM_CONTIGS = len(sc.CONTIGS)


class Malformed(Exception):
    """recount: the slice of query .query breaks the layout (args[0])."""

    @property
    def query(self):
        return self.args[0]


class Summary:
    def __init__(self, num_queries, num_aligned, alignments, total_aligned_length, num_indels, unaligned, penalties):
        self.num_queries, self.num_aligned, self.total_aligned_length, self.num_indels = num_queries, num_aligned, total_aligned_length, num_indels
        self.alignments = alignments  # per query
        self.num_alignments = int(sum(alignments))
        self.unaligned = np.array(unaligned, np.int64)
        self.num_unaligned = len(unaligned)
        self.penalties = np.array(penalties, np.float64)

    def close(self):
        pass


def recount(arrays, num_contigs=NUM_CONTIGS, nq=None):
    """The summary of the first nq queries of the four streams, or Malformed(lowest malformed query): an int that would be read at or behind the end of
    the query's slice, nseq outside 1 .. 2, nb < 1, a contig outside the index."""
    ints, dbls, io, do = arrays
    nq = len(io) - 1 if nq is None else nq
    aligned = length = indels = 0
    per_query, unaligned, penalties = [], [], []
    for q in range(nq):
        sl, dl = [int(x) for x in ints[io[q]:io[q + 1]]], dbls[do[q]:do[q + 1]]
        at = dat = n_al = 0
        mine = []
        try:
            ncomp = sl[at]; at += 1
            for _ in range(ncomp):
                nal = sl[at]; at += 1
                for _ in range(nal):
                    nseq = sl[at + 1]; at += 2
                    if dat + 4 > len(dl):
                        raise IndexError
                    mine.append(dl[dat + 3]); dat += 4
                    if not 1 <= nseq <= 2:
                        raise IndexError
                    for _ in range(nseq):
                        contig, nb = sl[at], sl[at + 2]
                        if nb < 1 or not 0 <= contig < num_contigs or at + 3 + 4 * nb > len(sl) or dat + 2 > len(dl):
                            raise IndexError
                        for j in range(nb):
                            la, lb = sl[at + 3 + 4 * j + 2], sl[at + 3 + 4 * j + 3]
                            length += la
                            indels += la != lb
                        at += 3 + 4 * nb; dat += 2
                    n_al += 1
        except IndexError:
            raise Malformed(q) from None
        per_query.append(n_al)
        penalties += mine
        if n_al:
            aligned += 1
        else:
            unaligned.append(q)
    return Summary(nq, aligned, per_query, length, indels, unaligned, penalties)


def arrays_of(streams):
    return streams.arrays() if isinstance(streams, sc.Streams) else streams


def first_queries(arrays, nq):
    """The streams of the first nq queries."""
    ints, dbls, io, do = arrays
    return ints[:io[nq]], dbls[:do[nq]], io[:nq + 1], do[:nq + 1]


def write_streams(path, arrays, num_contigs=NUM_CONTIGS):
    ints, dbls, io, do = arrays
    with open(path, "wb") as f:
        f.write(np.array([len(io) - 1, len(ints), len(dbls), num_contigs], np.int64).tobytes())
        for a, t in ((ints, np.int32), (dbls, np.float64), (io, np.int64), (do, np.int64)):
            f.write(np.ascontiguousarray(a, dtype=t).tobytes())
    return path


def bits(x):
    return struct.pack("<d", float(x))


def same(got, want, want_unaligned=True):
    """got (an api.BatchSummary, or anything of its shape) equals want (a Summary): the counts, the list, and the penalties bit for bit."""
    assert (got.num_queries, got.num_aligned, got.num_alignments, got.total_aligned_length, got.num_indels) == \
           (want.num_queries, want.num_aligned, want.num_alignments, want.total_aligned_length, want.num_indels)
    assert np.asarray(got.penalties, np.float64).tobytes() == want.penalties.tobytes()
    if want_unaligned:
        assert got.num_unaligned == want.num_unaligned and list(got.unaligned) == list(want.unaligned)
    else:
        assert got.num_unaligned == 0 and len(got.unaligned) == 0
    return True


def many_alignments_case(nq, at, n=40):
    """nq single reads, all unaligned but query `at`, which has n alignments with penalties that no two share."""
    s = sc.Streams()
    for q in range(nq):
        if q == at:
            s.aligned([(0.0, 0.1 * k + 1e-9 * k * k, [(k % NUM_CONTIGS, k % 2, sc.blocks_of(50, [("M", 20), ("I", 1 + k % 3), ("M", 20)], start_b=100 * k))]) for k in range(n)])
        else:
            s.unaligned()
    return s


def none_unaligned_case(nq):
    s = sc.Streams()
    for q in range(nq):
        s.aligned([(0.0, 0.5 + q, [(q % NUM_CONTIGS, q % 2, sc.whole(30, q))])])
    return s
