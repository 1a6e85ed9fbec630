"""Synthetic batches with qualities for the tests of the unaligned-query file's text (tests/test_unaligned_rules.py on the CPU, tests/test_gpu_unaligned.py on
the GPU): generated here, no fixture files.  Batch extends sam_cases.Batch with quals / qual_off / has_qual over sam_cases.Streams; expected() is the yardstick,
the unaligned-query file and the statistics that hostio.Writer (xmio_write_batch) makes of the same batch and streams; write_case() is the file
tests/unaligned_rules_main.cpp reads."""
import ctypes as C
import struct
import tempfile

import numpy as np

import sam_cases as sc
from mapper_amd import hostio


class Batch(sc.Batch):
    def __init__(self, reads, names, quals=None):
        """reads, names: as sam_cases.Batch.  quals: per query a tuple of one entry per mate - bytes (the mate came as FASTQ) or None (as FASTA); None for the
        whole batch: a batch without qualities (quals, qual_off and has_qual are NULL, as a reader without keep_qualities leaves them)."""
        super().__init__(reads, names)
        n = self.num_queries
        self.has_qual = self.qual_off = self.quals = None
        if quals is None:
            return
        self.has_qual = np.zeros(2 * n, np.uint8)
        self.qual_off = np.zeros(2 * n + 1, np.int64)
        text = []
        for q in range(n):
            for m in range(2):
                given = quals[q][m] if m < len(reads[q]) else None
                self.has_qual[2 * q + m] = 1 if given is not None else 0
                text.append(bytes(given) if given is not None else b"")
                self.qual_off[2 * q + m + 1] = self.qual_off[2 * q + m] + len(text[-1])
        self.quals = b"".join(text)
        self._quals = C.create_string_buffer(self.quals, max(len(self.quals), 1))
        self._raw.quals = C.addressof(self._quals)
        self._raw.qual_off = self.qual_off.ctypes.data_as(C.POINTER(C.c_int64))
        self._raw.has_qual = self.has_qual.ctypes.data_as(C.POINTER(C.c_uint8))


def stats_bits(st):
    return (st.num_queries, st.num_aligned, st.total_aligned_length, st.num_indels, struct.pack("<d", st.total_penalty))


def expected(batch, streams, contigs=sc.CONTIGS):
    """The host path: hostio.Writer's unaligned-query file for the batch and the streams (a Streams or its four arrays) and its statistics bit for bit;
    RuntimeError with the library's message on malformed streams."""
    arrays = streams.arrays() if isinstance(streams, sc.Streams) else streams
    with tempfile.TemporaryFile("w+b") as f:
        w = hostio.Writer(contigs, None, f, threads=2)
        w.write(batch, sc.Result(arrays))
        f.seek(0)
        return f.read(), stats_bits(w.stats)


def write_case(path, batch, streams, contigs=sc.CONTIGS):
    ints, dbls, io, do = streams.arrays() if isinstance(streams, sc.Streams) else streams
    with_qual = batch.has_qual is not None
    head = np.array([batch.num_queries, batch.codes_length, len(batch.names), len(batch.quals) if with_qual else 0, 1 if with_qual else 0, len(ints), len(dbls), len(contigs)], np.int64)
    parts = [head, batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes[:batch.codes_length], batch.names, batch.name_off]
    if with_qual:
        parts += [batch.quals, batch.qual_off, batch.has_qual]
    parts += [ints, dbls, io, do]
    with open(path, "wb") as f:
        for part in parts:
            f.write(part if isinstance(part, bytes) else np.ascontiguousarray(part).tobytes())
    return path


def quality(rng, n):
    return bytes(rng.integers(33, 127, n).astype(np.uint8))


def with_qualities(batch, seed, share=0.5, per_mate=False):
    """The reads and names of a sam_cases.Batch again, a share of the queries (per_mate: of the mates, each on its own) as FASTQ -> Batch."""
    rng = np.random.default_rng(seed)
    reads = [tuple(batch.codes[batch.mate_offset[2 * q + m]:batch.mate_offset[2 * q + m] + batch.mate_length[2 * q + m]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    names = [tuple(batch.names[batch.name_off[2 * q + m]:batch.name_off[2 * q + m + 1]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    quals = []
    for r in reads:
        fq = rng.random() < share
        quals.append(tuple(quality(rng, len(m)) if (rng.random() < share if per_mate else fq) else None for m in r))
    return Batch(reads, names, quals)


def random_case(seed, nq, read_len=None, name_len=None, unaligned=0.2, qualities=0.5):
    """sam_cases.random_case with qualities for a share of its queries (None: a batch without qualities)."""
    batch, streams = sc.random_case(seed, nq, read_len=read_len, name_len=name_len, unaligned=unaligned)
    if qualities is None:
        reads = [tuple(batch.codes[batch.mate_offset[2 * q + m]:batch.mate_offset[2 * q + m] + batch.mate_length[2 * q + m]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
        names = [tuple(batch.names[batch.name_off[2 * q + m]:batch.name_off[2 * q + m + 1]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
        return Batch(reads, names, None), streams
    return with_qualities(batch, seed, qualities), streams


def aligned(s, length):
    return s.aligned([(0.0, 1.0, [(0, 0, sc.whole(length))])])


def shapes_case(every=None):
    """Every shape of the test plan once, by hand: FASTQ mates, FASTA mates, pairs of one mate each (FASTQ first and FASTA first), both mates FASTQ, both FASTA;
    names of 0 and of 300 bytes; a mate of 1 base and a mate of 30 000 bases (with qualities); all 16 base codes; aligned queries between the unaligned ones.
    every: None - as described; True - every query unaligned; False - none."""
    rng = np.random.default_rng(31)
    reads, names, quals, s, kinds = [], [], [], sc.Streams(), []

    def add(mates, mate_names, mate_quals, unaligned=True):
        reads.append(tuple(mates)); names.append(tuple(mate_names)); quals.append(tuple(mate_quals))
        kinds.append(unaligned)

    all16 = np.arange(16, dtype=np.uint8)
    r = sc.read_of(rng, 40); add([r], [b"fastq_single"], [quality(rng, 40)])
    r = sc.read_of(rng, 35); add([r], [b"aligned_between"], [quality(rng, 35)], unaligned=False)
    r = sc.read_of(rng, 40); add([r], [b"fasta_single"], [None])
    add([sc.read_of(rng, 30), sc.read_of(rng, 31)], [b"pair_fq_fa/1", b"pair_fq_fa/2"], [quality(rng, 30), None])
    add([sc.read_of(rng, 30), sc.read_of(rng, 31)], [b"pair_fa_fq/1", b"pair_fa_fq/2"], [None, quality(rng, 31)])
    add([sc.read_of(rng, 28), sc.read_of(rng, 29)], [b"pair_fq_fq/1", b"pair_fq_fq/2"], [quality(rng, 28), quality(rng, 29)])
    add([sc.read_of(rng, 28), sc.read_of(rng, 29)], [b"pair_fa_fa/1", b"pair_fa_fa/2"], [None, None])
    add([sc.read_of(rng, 20), sc.read_of(rng, 21)], [b"pair_aligned/1", b"pair_aligned/2"], [quality(rng, 20), quality(rng, 21)], unaligned=False)
    add([sc.read_of(rng, 17)], [b""], [quality(rng, 17)])
    add([sc.read_of(rng, 17)], [b""], [None])
    add([sc.read_of(rng, 19)], [b"n" * 300], [quality(rng, 19)])
    add([sc.read_of(rng, 1)], [b"one_base"], [b"!"])
    add([sc.read_of(rng, 1)], [b"one_base_fasta"], [None])
    add([all16], [b"sixteen_codes"], [quality(rng, 16)])
    add([np.concatenate([all16[::-1], all16])], [b"sixteen_codes_twice"], [None])
    add([rng.integers(0, 16, 30_000).astype(np.uint8)], [b"thirty_thousand"], [quality(rng, 30_000)])
    add([sc.read_of(rng, 12)], [b"last_aligned"], [None], unaligned=False)
    add([sc.read_of(rng, 12)], [b"last"], [quality(rng, 12)])
    for q, unaligned in enumerate(kinds):
        if every is True or (every is None and unaligned):
            s.unaligned()
        elif len(reads[q]) == 2:
            s.aligned([(0.4, 2.5, [(0, 0, sc.whole(len(reads[q][0]))), (1, 1, sc.whole(len(reads[q][1]), 7))])])
        else:
            aligned(s, len(reads[q][0]))
    return Batch(reads, names, quals), s


def without_has_qual(batch):
    """The same reads and names as a batch without qualities (has_qual == NULL)."""
    reads = [tuple(batch.codes[batch.mate_offset[2 * q + m]:batch.mate_offset[2 * q + m] + batch.mate_length[2 * q + m]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    names = [tuple(batch.names[batch.name_off[2 * q + m]:batch.name_off[2 * q + m + 1]] for m in range(batch.mate_count[q])) for q in range(len(batch))]
    return Batch(reads, names, None)


def tile_edge_case(tile, tiles=9):
    """The pattern of sam_cases.tile_edge_case for the unaligned-query file: unaligned single reads whose names are as long as it takes for the records to end
    at -1, 0 and +1 of the multiples of `tile`, one multiple after the other, with a short record behind each so that records also start there, FASTQ and FASTA
    in turn, and an aligned query between them now and then.  -> (batch, streams, the ends asked for)"""
    rng = np.random.default_rng(36)
    fq_base, fa_base = 1 + 1 + 50 + 1 + 2 + 50 + 1, 1 + 1 + 50 + 1   # a record of 50 bases with an empty name
    reads, names, quals, s, at, ends = [], [], [], sc.Streams(), 0, []
    for k in range(1, tiles + 1):
        fq = k % 2 == 1
        target = k * tile + (k % 3 - 1)
        pad = target - at - (fq_base if fq else fa_base)
        assert pad >= 0
        reads.append((sc.read_of(rng, 50),)); names.append((b"q" * pad,)); quals.append((quality(rng, 50) if fq else None,)); s.unaligned()
        at = target
        ends.append(target)
        if k % 4 == 0:
            reads.append((sc.read_of(rng, 50),)); names.append((b"aligned",)); quals.append((None,)); aligned(s, 50)
        reads.append((sc.read_of(rng, 50),)); names.append((b"s",)); quals.append((None if fq else quality(rng, 50),)); s.unaligned()
        at += (fa_base if fq else fq_base) + 1
    return Batch(reads, names, quals), s, ends


def one_between(nq=4097, at=2048):
    """One unaligned query (FASTQ, 150 bases) between nq - 1 aligned ones."""
    rng = np.random.default_rng(37)
    reads = [(sc.read_of(rng, 150 if q == at else 24),) for q in range(nq)]
    names = [(b"q%d" % q,) for q in range(nq)]
    quals = [(quality(rng, len(r[0])),) for r in reads]
    s = sc.Streams()
    for q in range(nq):
        if q == at:
            s.unaligned()
        else:
            aligned(s, 24)
    return Batch(reads, names, quals), s


# ---------------------------------------------------------------- real alignments: a small reference and reads of which every fifth aligns nowhere
REAL_REFERENCE_LENGTH = 60_000
DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)


def real_reference():
    from mapper_amd import synth
    return [("chrR", synth.synthetic_reference(REAL_REFERENCE_LENGTH, seed=0xEC011))]


def real_reads(n, seed=41, pairs=False):
    """n queries of 100 to 150 bases a mate.  Query i with i % 5 == 4 is random bases (both mates of a pair): a random read of 100 bases and more has no
    alignment within the default error rate on a random reference of 60 000 bases.  Every other query is cut from the reference, on either strand, with at
    most one substituted base a mate (for a pair: mate 2 from the opposite strand, 100 bases further on), which always aligns.  So exactly the queries with
    i % 5 == 4 - a fifth - are unaligned.  -> list of tuples of code arrays"""
    from mapper_amd import synth
    rng = np.random.default_rng(seed)
    ref = real_reference()[0][1]
    out = []
    for i in range(n):
        lens = [int(rng.integers(100, 151)) for _ in range(2 if pairs else 1)]
        if i % 5 == 4:
            out.append(tuple(sc.read_of(rng, k) for k in lens))
            continue
        at = int(rng.integers(0, len(ref) - 500))
        mates = [ref[at:at + lens[0]].copy()]
        if pairs:
            start = at + lens[0] + 100
            mates.append(synth.revcomp_codes(ref[start:start + lens[1]]).copy())
        elif rng.random() < 0.5:
            mates[0] = synth.revcomp_codes(mates[0]).copy()
        for m in mates:
            if rng.random() < 0.5:
                k = int(rng.integers(0, len(m)))
                m[k] = np.uint8(1 << ((int(m[k]).bit_length() % 4)))  # another one of A, C, G, T
        out.append(tuple(mates))
    return out


def fastq_text(reads, mate, name, seed):
    """The mates `mate` of the reads as four-line FASTQ records with random qualities."""
    rng = np.random.default_rng(seed)
    return b"".join(b"@" + (name % i).encode() + b" comment\n" + DEC[r[mate]].tobytes() + b"\n+\n" + quality(rng, len(r[mate])) + b"\n" for i, r in enumerate(reads))


def fasta_text(reads, mate, name, width=60):
    """The same as FASTA records wrapped at `width` letters."""
    out = []
    for i, r in enumerate(reads):
        text = DEC[r[mate]].tobytes()
        out.append(b">" + (name % i).encode() + b" comment\n" + b"".join(text[k:k + width] + b"\n" for k in range(0, len(text), width)))
    return b"".join(out)
