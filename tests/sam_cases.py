"""Synthetic batches and result streams for the SAM formatter's tests (tests/test_sam_rules.py on the CPU, tests/test_gpu_sam.py on the GPU): generated here,
no fixture files.  A Batch has the shape hostio.Writer.write and api.ReferenceDatabase.format_sam_last read (a _ptr to a hostio.XmioBatch); Streams builds the
four result streams of include/xmapper_hip.h:73-82 query by query; expected() is the yardstick, hostio.Writer's bytes for the same input; write_case() is the
file tests/sam_rules_main.cpp reads."""
import ctypes as C
import tempfile

import numpy as np

from mapper_amd import hostio

CONTIGS = ["c", "chr2", "a_contig_with_a_rather_long_name.1", "chrUn_KI270302v1"]
TOP = 2**31 - 1


class Batch:
    def __init__(self, reads, names):
        """reads: per query a tuple of one or two uint8 code arrays; names: per query a tuple of as many bytes objects."""
        n = len(reads)
        self.num_queries = n
        self.mate_count = np.array([len(r) for r in reads], np.int32)
        self.mate_offset = np.zeros(2 * n, np.int64)
        self.mate_length = np.zeros(2 * n, np.int32)
        self.name_off = np.zeros(2 * n + 1, np.int64)
        chunks, text, at = [], [], 0
        for q in range(n):
            for m in range(2):
                if m < len(reads[q]):
                    self.mate_offset[2 * q + m], self.mate_length[2 * q + m] = at, len(reads[q][m])
                    chunks.append(np.asarray(reads[q][m], np.uint8))
                    at += len(reads[q][m])
                    text.append(bytes(names[q][m]))
                self.name_off[2 * q + m + 1] = self.name_off[2 * q + m] + (len(names[q][m]) if m < len(reads[q]) else 0)
        self.codes = np.concatenate(chunks) if chunks else np.zeros(1, np.uint8)
        self.codes_length = at
        self.names = b"".join(text)
        self._names = C.create_string_buffer(self.names, max(len(self.names), 1))
        as_ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        self._raw = hostio.XmioBatch(n, as_ptr(self.mate_count, C.c_int32), as_ptr(self.mate_offset, C.c_int64), as_ptr(self.mate_length, C.c_int32), as_ptr(self.codes, C.c_uint8), at,
                                     C.addressof(self._names), as_ptr(self.name_off, C.c_int64), None, None, None, None)
        self._ptr = C.pointer(self._raw)

    def __len__(self):
        return self.num_queries


def blocks_of(length, ops, lead=0, start_b=1000):
    """Blocks (startA, startB, lengthA, lengthB) from `lead` on: ops is a list of ('M' | 'I' | 'D', n); the rest of `length` behind them is a trailing soft clip."""
    out, a, b = [], lead, start_b
    for op, n in ops:
        out.append((a, b, n if op != "D" else 0, n if op != "I" else 0))
        a += n if op != "D" else 0
        b += n if op != "I" else 0
    assert a <= length and out
    return out


def whole(length, start_b=1000):
    return blocks_of(length, [("M", length)], 0, start_b)


class Streams:
    def __init__(self):
        self.ints, self.dbls, self.int_off, self.dbl_off = [], [], [0], [0]

    def _seq(self, contig, rev, blocks, penalties=(0.0, 0.0)):
        self.ints += [contig, rev, len(blocks)] + [int(x) for b in blocks for x in b]
        self.dbls += list(penalties)

    def _end(self):
        self.int_off.append(len(self.ints)); self.dbl_off.append(len(self.dbls))
        return self

    def unaligned(self):
        self.ints += [1, 0]
        return self._end()

    def aligned(self, alignments):
        """One component.  alignments: list of (spacing penalty, penalty, [(contig, rev, blocks), ...]) - one sequence for a single read, two for a pair."""
        self.ints += [1, len(alignments)]
        for spacing, penalty, seqs in alignments:
            self.ints += [17, len(seqs)]
            self.dbls += [spacing, 1.0, 0.0, penalty]
            for s in seqs:
                self._seq(*s)
        return self._end()

    def fallback(self, per_mate):
        """A pair that fell back: two components; per_mate: for each mate a list of (penalty, (contig, rev, blocks))."""
        self.ints.append(2)
        for als in per_mate:
            self.ints.append(len(als))
            for penalty, s in als:
                self.ints += [0, 1]
                self.dbls += [0.0, 1.0, 0.0, penalty]
                self._seq(*s)
        return self._end()

    def raw(self, ints, dbls):
        self.ints += list(ints); self.dbls += list(dbls)
        return self._end()

    def arrays(self):
        return np.array(self.ints, np.int32), np.array(self.dbls, np.float64), np.array(self.int_off, np.int64), np.array(self.dbl_off, np.int64)


class Result:
    def __init__(self, arrays):
        self.ints, self.dbls, self.int_off, self.dbl_off = arrays


def expected(batch, streams, contigs=CONTIGS):
    """hostio.Writer's SAM bytes for the batch and the streams (a Streams or its four arrays); RuntimeError with the library's message on malformed streams."""
    arrays = streams.arrays() if isinstance(streams, Streams) else streams
    with tempfile.TemporaryFile("w+b") as f:
        hostio.Writer(contigs, f, None, threads=2).write(batch, Result(arrays))
        f.seek(0)
        return f.read()


def write_case(path, batch, streams, contigs=CONTIGS):
    ints, dbls, io, do = streams.arrays() if isinstance(streams, Streams) else streams
    names = b"".join(c.encode() for c in contigs)
    off = np.cumsum([0] + [len(c.encode()) for c in contigs]).astype(np.int64)
    head = np.array([batch.num_queries, batch.codes_length, len(batch.names), len(ints), len(dbls), len(contigs), len(names), 0], np.int64)
    with open(path, "wb") as f:
        for part in (head, batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes[:batch.codes_length], batch.names, batch.name_off, ints, dbls, io, do, names, off):
            f.write(part if isinstance(part, bytes) else np.ascontiguousarray(part).tobytes())
    return path


def read_of(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


def shapes_case():
    """Every shape of the test plan once, by hand: single reads on both strands, pairs in the four strand combinations, fallback pairs with 0, 1 and 2 alignments
    per component, one to three alignments per query, unaligned queries between aligned ones, soft clips, equal-length blocks that merge, insertions and
    deletions (also next to each other), the sixteen codes on both strands, names of 0, 1 and 200 bytes, contigs with names of several lengths, positions up
    to 2^31 - 1."""
    rng = np.random.default_rng(11)
    reads, names, s = [], [], Streams()

    def single(read, name, *al):
        reads.append((read,)); names.append((name,))
        return read

    all16 = np.arange(16, dtype=np.uint8)
    r = single(read_of(rng, 40), b"fwd"); s.aligned([(0.0, 0.0, [(0, 0, whole(40))])])
    r = single(read_of(rng, 40), b"rev"); s.aligned([(0.0, 1.5, [(1, 1, whole(40, 7))])])
    single(read_of(rng, 30), b"unaligned_1"); s.unaligned()
    single(all16, b"codes_fwd"); s.aligned([(0.0, 2.1, [(2, 0, whole(16))])])
    single(np.concatenate([all16, all16[:5]]), b"codes_rev"); s.aligned([(0.0, 0.6000000000000001, [(3, 1, whole(21))])])
    single(read_of(rng, 50), b""); s.aligned([(0.0, 7.300000000000001, [(0, 0, blocks_of(50, [("M", 40)], lead=4))])])                    # both soft clips, empty name
    single(read_of(rng, 50), b"x"); s.aligned([(0.0, 1e-4, [(1, 0, blocks_of(50, [("M", 10), ("M", 10), ("M", 30)]))])])                  # three blocks, one M
    single(read_of(rng, 60), b"n" * 200); s.aligned([(0.0, 123456789.5, [(2, 1, blocks_of(60, [("M", 10), ("I", 3), ("D", 4), ("M", 5), ("D", 2), ("D", 1), ("I", 1), ("I", 2), ("M", 30)], lead=2))])])
    single(read_of(rng, 25), b"three"); s.aligned([(0.0, float(k), [(k, k % 2, whole(25, 100 * k))]) for k in range(3)])
    single(read_of(rng, 25), b"two"); s.aligned([(0.0, 0.5, [(3, 0, whole(25, TOP - 30))]), (0.0, 1e7, [(3, 1, whole(25, TOP))])])  # POS up to 2^31
    single(read_of(rng, 1), b"unaligned_2"); s.unaligned()
    for k, (r1, r2) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        reads.append((read_of(rng, 33), read_of(rng, 27))); names.append((b"pair%d/1" % k, b"pair%d/2" % k))
        s.aligned([(0.4 * k, 2.5 + k, [(k % 4, r1, blocks_of(33, [("M", 30)], lead=1, start_b=500 + k)), ((k + 1) % 4, r2, blocks_of(27, [("M", 7), ("D", 2), ("M", 20)], start_b=TOP - 40))])])
    reads.append((read_of(rng, 20), read_of(rng, 22))); names.append((b"pair_two_alignments/1", b""))
    s.aligned([(0.0, 1.0, [(0, 0, whole(20)), (0, 1, whole(22, 300))]), (9.999999999999999e-4, 3.0, [(1, 1, whole(20)), (2, 0, whole(22, 5))])])
    for k, (n1, n2) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (0, 2), (2, 2), (1, 2))):
        reads.append((read_of(rng, 18), read_of(rng, 19))); names.append((b"fb%d/1" % k, b"fb%d/2" % k))
        s.fallback([[(3.5 + i, (i % 4, (i + k) % 2, whole(18, 40 + i))) for i in range(n1)], [(12.25, ((i + 1) % 4, i % 2, blocks_of(19, [("M", 9), ("I", 1), ("M", 9)], start_b=900))) for i in range(n2)]])
    single(read_of(rng, 12), b"last"); s.aligned([(0.0, 10.0, [(0, 1, whole(12, 0))])])
    return Batch(reads, names), s


def random_case(seed, nq, read_len=None, name_len=None, unaligned=0.2):
    """nq queries of every kind at random.  read_len / name_len: a fixed length for every mate / name (None: mixed)."""
    rng = np.random.default_rng(seed)
    reads, names, s = [], [], Streams()
    n_contigs = len(CONTIGS)

    def seq_al(length):
        blocks = []
        a = int(rng.integers(0, 4)) if rng.random() < 0.3 and length > 4 else 0
        bpos = int(rng.integers(0, 200000))
        end = length - (int(rng.integers(0, 4)) if rng.random() < 0.3 and length > 8 else 0)
        while a < end:
            kind = rng.random()
            n = int(rng.integers(1, max(2, end - a + 1)))
            if kind < 0.6 or not blocks:
                blocks.append((a, bpos, n, n)); a += n; bpos += n
            elif kind < 0.8:
                n = min(n, 5); blocks.append((a, bpos, n, 0)); a += n
            else:
                n = min(n, 7); blocks.append((a, bpos, 0, n)); bpos += n
        return (int(rng.integers(0, n_contigs)), int(rng.integers(0, 2)), blocks)

    penalties = [0.0, 1.0, 2.6, 7.300000000000001, 10.0, 1e-4, 123456789.5, 0.6000000000000001, 3.5, 12.25]
    for q in range(nq):
        paired = rng.random() < 0.4
        lens = [read_len if read_len is not None else int(rng.integers(1, 160)) for _ in range(2 if paired else 1)]
        reads.append(tuple((1 << rng.integers(0, 4, n)).astype(np.uint8) if rng.random() < 0.9 else rng.integers(0, 16, n).astype(np.uint8) for n in lens))
        nl = name_len if name_len is not None else int(rng.integers(0, 40))
        names.append(tuple((b"%d/%d_" % (q, m) + b"n" * nl)[:nl] for m in range(len(lens))))
        mode = rng.random()
        if mode < unaligned:
            s.unaligned()
        elif paired and mode < unaligned + 0.2:
            s.fallback([[(float(rng.choice(penalties)), seq_al(lens[m])) for _ in range(int(rng.integers(0, 3)))] for m in range(2)])
        else:
            s.aligned([(float(rng.choice([0.0, 0.4, 1.0])) if paired else 0.0, float(rng.choice(penalties)), [seq_al(n) for n in lens]) for _ in range(int(rng.integers(1, 4)))])
    return Batch(reads, names), s


def all_unaligned_case(nq):
    rng = np.random.default_rng(3)
    s = Streams()
    for _ in range(nq):
        s.unaligned()
    return Batch([(read_of(rng, 10),) for _ in range(nq)], [(b"u%d" % q,) for q in range(nq)]), s


def three_alignments_case():
    rng = np.random.default_rng(4)
    s = Streams().aligned([(0.0, 1.0 + k, [(k, k % 2, whole(70, 10 * k))]) for k in range(3)])
    return Batch([(read_of(rng, 70),)], [(b"only",)]), s


def one_pair_case():
    """One pair alignment with an indel in each mate: the slice the cut test shortens."""
    rng = np.random.default_rng(5)
    s = Streams().aligned([(0.4, 2.5, [(0, 0, blocks_of(33, [("M", 10), ("I", 2), ("M", 20)], lead=1)), (1, 1, blocks_of(27, [("M", 7), ("D", 2), ("M", 20)]))])])
    return Batch([(read_of(rng, 33), read_of(rng, 27))], [(b"p/1", b"p/2")]), s


def tile_edge_case(tile, tiles=9):
    """Single reads whose names are as long as it takes for the records to end at -1, 0 and +1 of the multiples of `tile`, one multiple after the other, with a
    short record behind each so that records also start there.  -> (batch, streams, the ends asked for)"""
    rng = np.random.default_rng(6)
    probe = Batch([(read_of(rng, 50),)], [(b"",)])
    al = lambda: [(0.0, 1.0, [(1, 0, whole(50, 12345))])]  # noqa: E731
    base = len(expected(probe, Streams().aligned(al())))  # a record with an empty name
    reads, names, s, at, ends = [], [], Streams(), 0, []
    for k in range(1, tiles + 1):
        for target in (k * tile + (k % 3 - 1), ):
            pad = target - at - base
            assert pad >= 0
            reads.append((read_of(rng, 50),)); names.append((b"q" * pad,)); s.aligned(al())
            at = target
            ends.append(target)
        reads.append((read_of(rng, 50),)); names.append((b"s",)); s.aligned(al())
        at += base + 1
    return Batch(reads, names), s, ends


def malformed_cases():
    """name -> (batch, streams, the query that is malformed): each of the six conditions in query 2 of five, and a second malformed query behind it (4), which
    must not be the one reported."""
    rng = np.random.default_rng(7)
    good_single = lambda s: s.aligned([(0.0, 1.0, [(0, 0, whole(20))])])  # noqa: E731
    bad = {
        "nseq_0": ([1, 1, 17, 0], [0.0, 1.0, 0.0, 1.0]),
        "nseq_3": ([1, 1, 17, 3] + [0, 0, 1, 0, 5, 20, 20] * 3, [0.0, 1.0, 0.0, 1.0] + [0.0] * 6),
        "nb_0": ([1, 1, 17, 1, 0, 0, 0], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),
        "contig_negative": ([1, 1, 17, 1, -1, 0, 1, 0, 5, 20, 20], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),
        "contig_too_large": ([1, 1, 17, 1, len(CONTIGS), 0, 1, 0, 5, 20, 20], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),
        "cursor_past_the_end": ([1, 1, 17, 1, 0, 0, 3, 0, 5, 20, 20], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),       # three blocks announced, one there
        "mate_beyond_the_query": ([1, 1, 17, 2, 0, 0, 1, 0, 5, 20, 20, 0, 0, 1, 0, 9, 20, 20], [0.0, 1.0, 0.0, 1.0] + [0.0] * 4),  # two sequences for a single read
        "third_component": ([3, 0, 0, 1, 17, 1, 0, 0, 1, 0, 5, 20, 20], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),    # mate 2 of a query that has one
        "pair_with_one_sequence": None,
    }
    out = {}
    for name, spec in bad.items():
        s = Streams()
        reads = [(read_of(rng, 20),) for _ in range(5)]
        names = [(b"m%d" % q,) for q in range(5)]
        good_single(s); s.unaligned()
        if spec is None:  # a paired query, one component, an alignment of one sequence
            reads[2] = (read_of(rng, 20), read_of(rng, 20)); names[2] = (b"m2/1", b"m2/2")
            s.raw([1, 1, 17, 1, 0, 0, 1, 0, 5, 20, 20], [0.0, 1.0, 0.0, 1.0, 0.0, 0.0])
        else:
            s.raw(*spec)
        good_single(s)
        s.raw([1, 1, 17, 0], [0.0, 1.0, 0.0, 1.0])
        out[name] = (Batch(reads, names), s, 2)
    return out
