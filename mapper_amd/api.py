"""Host-side mirror of the reference's programmatic API for the seed-and-extend path.

Mirrors src/main/java/mapper/Api.java:18-107 (newDatabase / align / alignOnce), AlignmentParameters.java:8-35 and the
Query / QueryAlignment / SequenceAlignment / AlignedBlock result types the Java host consumes, on top of the C ABI of
include/xmapper_hip.h.  Everything is aligned on the GPU by libxmapper_hip.so; there is no CPU path.
"""
import ctypes as C
import os
import time
import numpy as np

from . import _capi, hostio

_CODE = np.full(256, 15, dtype=np.uint8)
for _ch, _v in {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}.items():
    _CODE[ord(_ch)] = _v
    _CODE[ord(_ch.lower())] = _v
_DECODE = "?ACMGRSVTWYHKDBN"
_COMP = np.array([((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3) for b in range(16)], dtype=np.uint8)


def encode(text):
    """IUPAC text -> 4-bit Basepairs codes, one per byte."""
    return _CODE[np.frombuffer(text.encode("ascii"), dtype=np.uint8)].copy()


def decode(codes):
    return "".join(_DECODE[int(c) & 15] for c in codes)


def reverse_complement(codes):
    return _COMP[np.asarray(codes, dtype=np.uint8)[::-1]]


class AlignmentParameters:
    """AlignmentParameters.java:8-35; defaults are Mapper.main's (Mapper.java:66-73, 409-453)."""

    def __init__(self, MutationPenalty=1.0, InsertionStart_Penalty=1.5, InsertionExtension_Penalty=0.5 + 0.1, DeletionStart_Penalty=1.5,
                 DeletionExtension_Penalty=0.5, MaxErrorRate=0.1, UnalignedPenalty=0.1, AmbiguityPenalty=0.1, MaxNumMatches=2**31 - 1,
                 Max_PenaltySpan=0.5):
        self.MutationPenalty = MutationPenalty
        self.InsertionStart_Penalty = InsertionStart_Penalty
        self.InsertionExtension_Penalty = InsertionExtension_Penalty
        self.DeletionStart_Penalty = DeletionStart_Penalty
        self.DeletionExtension_Penalty = DeletionExtension_Penalty
        self.MaxErrorRate = MaxErrorRate
        self.UnalignedPenalty = UnalignedPenalty
        self.AmbiguityPenalty = AmbiguityPenalty
        self.MaxNumMatches = MaxNumMatches
        self.Max_PenaltySpan = Max_PenaltySpan

    def _c(self):
        p = _capi.XmParams()
        for f, _ in _capi.XmParams._fields_:
            if f != "reserved":
                setattr(p, f, getattr(self, f))
        return p


class Query:
    """Query(seq) / Query(seq1, seq2, expectedInnerDistance, spacingDeviationPerUnitPenalty) [QuickVariants]."""

    def __init__(self, *sequences, expected_inner_distance=0.0, spacing_deviation_per_unit_penalty=1.0, name=None, names=None):
        self.sequences = [encode(s) if isinstance(s, str) else np.ascontiguousarray(s, dtype=np.uint8) for s in sequences]
        if not 1 <= len(self.sequences) <= 2:
            raise ValueError("a Query has 1 or 2 sequences")
        self.expected_inner_distance = float(expected_inner_distance)
        self.spacing_deviation_per_unit_penalty = float(spacing_deviation_per_unit_penalty)
        self.names = names or ([name] * len(self.sequences) if name else ["query"] * len(self.sequences))


class AlignedBlock:
    __slots__ = ("startA", "startB", "lengthA", "lengthB")

    def __init__(self, sa, sb, la, lb):
        self.startA, self.startB, self.lengthA, self.lengthB = sa, sb, la, lb


class SequenceAlignment:
    """SequenceAlignment [QuickVariants]: ordered AlignedBlocks + referenceReversed + penalties."""

    def __init__(self, contig, reference_reversed, blocks, total_penalty, aligned_penalty):
        self.contig, self.reference_reversed, self.sections = contig, bool(reference_reversed), blocks
        self.penalty, self.aligned_penalty = total_penalty, aligned_penalty

    def start_index_b(self):
        return self.sections[0].startB

    def end_index_b(self):
        return self.sections[-1].startB + self.sections[-1].lengthB

    def aligned_text(self, query_codes, ref_codes):
        """(getAlignedTextA, getAlignedTextB); query_codes must be the strand that was aligned."""
        a, b = [], []
        for s in self.sections:
            a.append(decode(query_codes[s.startA:s.startA + s.lengthA]) if s.lengthA > 0 else "-" * s.lengthB)
            b.append(decode(ref_codes[s.startB:s.startB + s.lengthB]) if s.lengthB > 0 else "-" * s.lengthA)
        return "".join(a), "".join(b)


class QueryAlignment:
    """QueryAlignment(components, spacingPenalty, overlapMultiplier, duplicationBonus, totalPenalty, innerDistance)
    (QueryMatch_Aligner.java:267)."""

    def __init__(self, components, spacing_penalty, overlap_multiplier, duplication_bonus, penalty, inner_distance):
        self.components = components
        self.spacing_penalty, self.overlap_multiplier, self.duplication_bonus = spacing_penalty, overlap_multiplier, duplication_bonus
        self.penalty, self.inner_distance = penalty, inner_distance


def decode_streams(ints, dbls, int_off, dbl_off, q):
    """-> QueryAlignments of query q as list (components) of lists of QueryAlignment."""
    ii = ints[int_off[q]:int_off[q + 1]]
    dd = dbls[dbl_off[q]:dbl_off[q + 1]]
    i = d = 0
    comps = []
    ncomp = int(ii[i]); i += 1
    for _ in range(ncomp):
        nal = int(ii[i]); i += 1
        als = []
        for _ in range(nal):
            inner, nseq = int(ii[i]), int(ii[i + 1]); i += 2
            sp, om, db, tp = (float(x) for x in dd[d:d + 4]); d += 4
            seqs = []
            for _ in range(nseq):
                contig, rev, nb = int(ii[i]), int(ii[i + 1]), int(ii[i + 2]); i += 3
                blocks = [AlignedBlock(int(ii[i + 4 * k]), int(ii[i + 4 * k + 1]), int(ii[i + 4 * k + 2]), int(ii[i + 4 * k + 3])) for k in range(nb)]
                i += 4 * nb
                seqs.append(SequenceAlignment(contig, rev, blocks, float(dd[d]), float(dd[d + 1])))
                d += 2
            als.append(QueryAlignment(seqs, sp, om, db, tp, inner))
        comps.append(als)
    return comps


class BatchResult:
    def __init__(self, d):
        self.__dict__.update(d)

    def __len__(self):
        return self.num_queries if "num_queries" in self.__dict__ else len(self.int_off) - 1

    @property
    def copies(self):
        """Queries of the batch whose results were copied from a byte-identical query instead of being aligned (xm_result.extra[7]; 0 unless
        ReferenceDatabase.set_collapse(True))."""
        return int(self.extra[7])

    @property
    def remembered(self):
        """Queries of the batch whose results were replayed from the context's memory of earlier batches instead of being aligned (xm_result.extra[6]; 0 unless
        ReferenceDatabase.set_memo(bytes) or ReferenceDatabase.attach_memory(QueryMemory))."""
        return int(self.extra[6])

    def query_alignments(self, q):
        if self.int_off is None:
            raise ValueError("this result has no streams: its context left them in HBM (ReferenceDatabase.set_result_copy(False)); use summary_last / format_sam_last, "
                             "or set_result_copy(True) before the align call")
        return decode_streams(self.ints, self.dbls, self.int_off, self.dbl_off, q)


class BatchSummary:
    """What ReferenceDatabase.summary_last computed on the GPU from the result streams of one batch: the five counts (num_queries, num_aligned, num_alignments,
    total_aligned_length, num_indels), `penalties` - every alignment's totalPenalty in stream order - and `unaligned` - the ascending indices of the queries
    without an alignment (empty unless asked for) - as numpy views of page-locked buffers of the library, and the milliseconds of the kernels and of the copy.
    close() gives the buffers back; the views must not be used after it."""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr
        t = ptr.contents
        self.num_queries, self.num_aligned, self.num_alignments = int(t.num_queries), int(t.num_aligned), int(t.num_alignments)
        self.total_aligned_length, self.num_indels, self.num_unaligned = int(t.total_aligned_length), int(t.num_indels), int(t.num_unaligned)
        self.kernel_ms, self.d2h_ms = t.kernel_ms, t.d2h_ms
        self.penalties = np.ctypeslib.as_array(t.penalties, shape=(self.num_alignments,)) if self.num_alignments else np.zeros(0, np.float64)
        self.unaligned = np.ctypeslib.as_array(t.unaligned, shape=(self.num_unaligned,)) if self.num_unaligned else np.zeros(0, np.int64)

    def close(self):
        if self._ptr is not None:
            self.penalties = self.unaligned = None
            self._L.xm_summary_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefsCount:
    """What ReferenceDatabase.refs_count_last counted on the GPU from the result streams of one batch: num_queries, num_aligned, `records` - one per combination
    of contigs, (tuple of ascending contig indices, queries with exactly that set) - and the queries the device left to the host (more than eight contigs, or
    a set whose fingerprint another set had taken): num_leftover_queries, and the contigs of their sequence alignments in leftover_contigs[leftover_offsets[k]:
    leftover_offsets[k + 1]].  counts() folds both into one dict.  Everything is copied out of the library's buffers here; close() gives them back."""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr
        t = ptr.contents
        self.num_queries, self.num_aligned = int(t.num_queries), int(t.num_aligned)
        self.num_combinations, self.num_leftover_queries = int(t.num_combinations), int(t.num_leftover_queries)
        self.kernel_ms, self.d2h_ms = t.kernel_ms, t.d2h_ms
        self.records = []
        if self.num_combinations:
            raw = np.ctypeslib.as_array(C.cast(t.records, C.POINTER(C.c_int32)), shape=(self.num_combinations, 12))  # count (two ints), n, ids[8], reserved
            count = raw[:, :2].copy().view(np.int64)[:, 0]
            self.records = [(tuple(int(x) for x in raw[k, 3:3 + int(raw[k, 2])]), int(count[k])) for k in range(self.num_combinations)]
        self.leftover_offsets, self.leftover_contigs = np.zeros(1, np.int64), np.zeros(0, np.int32)
        if self.num_leftover_queries:
            self.leftover_offsets = np.ctypeslib.as_array(t.leftover_offsets, shape=(self.num_leftover_queries + 1,)).copy()
            total = int(self.leftover_offsets[-1])
            self.leftover_contigs = np.ctypeslib.as_array(t.leftover_contigs, shape=(max(total, 1),))[:total].copy()
        self.close()

    def counts(self):
        """-> {tuple of ascending contig indices: queries}: the records, and every left-over query added to the set of its contigs."""
        out = {}
        for ids, count in self.records:
            out[ids] = out.get(ids, 0) + count
        lo = self.leftover_offsets
        for k in range(self.num_leftover_queries):
            ids = tuple(sorted(set(int(c) for c in self.leftover_contigs[lo[k]:lo[k + 1]])))
            out[ids] = out.get(ids, 0) + 1
        return out

    def close(self):
        if self._ptr is not None:
            self._L.xm_refs_count_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SamText:
    """The SAM records of one batch as ReferenceDatabase.format_sam_last built them: `bytes` of text (no header) in a page-locked buffer of the library, `records`
    lines, and the milliseconds of the call's three parts (names up, kernels, text down).  memoryview(text) / text.view() reads it without a copy, bytes(text)
    copies it; close() gives the buffer back."""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr
        t = ptr.contents
        self.bytes, self.records = int(t.bytes), int(t.records)
        self.h2d_ms, self.kernel_ms, self.d2h_ms = t.h2d_ms, t.kernel_ms, t.d2h_ms

    def view(self):
        if self._ptr is None:
            raise ValueError("the text has been closed")
        return memoryview((C.c_char * self.bytes).from_address(self._ptr.contents.text)).cast("B") if self.bytes else memoryview(b"")

    def __bytes__(self):
        return bytes(self.view())

    def __len__(self):
        return self.bytes

    def close(self):
        if self._ptr is not None:
            self._L.xm_sam_text_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check(rc, prefix=""):
    """A C entry that returns non-zero has left its message in xm_last_error."""
    if rc:
        raise RuntimeError(prefix + _capi.lib().xm_last_error().decode())


def index_cache_path(cache_dir, contigs, opts):
    """<cache_dir>/cache/<digest>/index.xmidx, the digest over the property text DirCache would hash (DirCache.java:19-60): the
    sequence database's keys (here: names, lengths and a digest of the bases) + enableGapmers, minInterestingSize, maxNumShortMatches,
    formatVersion, type (HashBlock_Database.java:106-114) + the duplication settings this library stores in the same file."""
    import hashlib
    seq = hashlib.sha256()
    for name, codes in contigs:
        seq.update(name.encode() + b"\0" + str(len(codes)).encode() + b"\0")
        seq.update(np.ascontiguousarray(codes, dtype=np.uint8).tobytes())
    props = {"sequences": seq.hexdigest(), "enableGapmers": str(bool(opts.enable_gapmers)).lower(), "minInterestingSize": str(opts.min_interesting_size),
             "maxNumShortMatches": "5", "formatVersion": "xmidx-1", "type": "HashBlock_Database",
             "duplications": "%d,%d,%d,%d" % (opts.dup_window, opts.dup_min_copies, opts.dup_min_length, opts.dup_max_length)}
    text = "{\n" + "".join('%s:"%s",\n' % (k, props[k]) for k in sorted(props)) + "}"
    d = os.path.join(os.fspath(cache_dir), "cache", hashlib.sha256(text.encode()).hexdigest()[:32])
    os.makedirs(d, exist_ok=True)
    meta = os.path.join(d, "metadata")
    if not os.path.exists(meta):
        with open(meta + ".tmp.%d" % os.getpid(), "w") as f:
            f.write(text)
        os.replace(meta + ".tmp.%d" % os.getpid(), meta)
    return os.path.join(d, "index.xmidx")


class ReferenceDatabase:
    """ReferenceDatabase.java: HashBlock_Database + DuplicationDetector of a reference, resident in HBM."""

    def __init__(self, contigs, mode="mapper", enable_gapmers=True, max_query_length=0, device=-1, host_only=False, dup=None, cache_dir=None, min_interesting_size=-1):
        """contigs: list of (name, IUPAC text or code array), already in Mapper.sortAndComplementReference order
        (use sort_reference()).  mode 'mapper' = Mapper.run assembly (duplication window 1000), 'api' = Api.newDatabase (window 1).
        cache_dir: --cache-dir (Mapper.java:264, DirCache.java:19-60): the index is read from / written to a file under
        <cache_dir>/cache/ that is named after the reference's cache keys (HashBlock_Database.java:106-114) and this build's settings."""
        self._L = _capi.lib()
        self.contigs = [(n, encode(s) if isinstance(s, str) else np.ascontiguousarray(s, dtype=np.uint8)) for n, s in contigs]
        ref, self._keep = _capi.make_ref(self.contigs)
        o = _capi.XmBuildOpts()
        o.enable_gapmers = 1 if enable_gapmers else 0
        o.min_interesting_size = int(min_interesting_size)  # (-1: from the reference's size, HashBlock_Database.java:52; tests pin the value a 3 Gb reference gets)
        o.max_hashed_length = int(max_query_length)
        o.dup_window = 1 if mode == "api" else 1000
        o.dup_min_copies = 2
        o.dup_min_length = o.dup_max_length = -1
        if dup:
            o.dup_min_length, o.dup_max_length, o.dup_min_copies, o.dup_window = dup
        o.device = device
        o.host_only = 1 if host_only else 0
        h = C.c_void_p()
        self.cache_file = None
        self.cache_hit = False
        if cache_dir is not None:
            self.cache_file = index_cache_path(cache_dir, self.contigs, o)
            if os.path.exists(self.cache_file) and self._L.xm_index_load(self.cache_file.encode(), C.byref(ref), C.byref(o), C.byref(h)) == 0:
                self._h = h
                self.cache_hit = True
                return
            # (a file that does not load - other settings behind the same name, truncated, older format - is rebuilt and replaced)
        _check(self._L.xm_index_build(C.byref(ref), C.byref(o), C.byref(h)))
        self._h = h
        if self.cache_file is not None:
            self.save(self.cache_file)

    def _tick(self, phase, seconds):
        """Host seconds this context has spent staging batches, in align calls and in format_sam_last (`seconds`: what the command line's phases sum up)."""
        held = self.__dict__.setdefault("seconds", {"stage": 0.0, "align": 0.0, "format": 0.0})
        held[phase] += seconds

    def save(self, path):
        """xm_index_save: the reference, every table hashed so far and the duplication map into one file."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        _check(self._L.xm_index_save(self._h, os.fspath(path).encode()))

    @classmethod
    def load(cls, path, device=-1, host_only=False, max_query_length=0):
        """xm_index_load without a build request to check against: whatever reference and settings the file holds."""
        self = cls.__new__(cls)
        self._L = _capi.lib()
        self.contigs, self._keep, self.cache_file, self.cache_hit = None, None, os.fspath(path), True
        o = _capi.XmBuildOpts()
        o.enable_gapmers = 1
        o.max_hashed_length = int(max_query_length)
        o.device = device
        o.host_only = 1 if host_only else 0
        h = C.c_void_p()
        _check(self._L.xm_index_load(os.fspath(path).encode(), None, C.byref(o), C.byref(h)))
        self._h = h
        return self

    def _sibling(self, create):
        """A further handle over this index: create(address of the new handle) is the C entry that makes it."""
        other = ReferenceDatabase.__new__(ReferenceDatabase)
        other._L = self._L
        other.contigs, other._keep, other.cache_file, other.cache_hit = self.contigs, self._keep, self.cache_file, self.cache_hit
        h = C.c_void_p()
        _check(create(C.byref(h)))
        other._h = h
        return other

    def replicate(self, device):
        """xm_index_replicate: a further context of this index on GPU `device`.  The host tables are shared; on another GPU the tables are copied
        HBM to HBM (nothing built or uploaded twice), on this index's own GPU the context reads the very same tables (= new_context)."""
        return self._sibling(lambda h: self._L.xm_index_replicate(self._h, int(device), h))

    def new_context(self):
        """xm_context_new: a further context on the same GPU - own stream, batch buffers, scratch and results over the same tables, as the reference's
        AlignerWorker threads share one HashBlock_Database through per-thread views (HashBlock_Database.java:129-133)."""
        return self._sibling(lambda h: self._L.xm_context_new(self._h, h))

    def set_scratch(self, nbytes):
        """xm_context_set_scratch: upper limit of the HBM this context allocates as scratch for its passes (0: the default)."""
        _check(self._L.xm_context_set_scratch(self._h, int(nbytes)))

    def set_collapse(self, enable):
        """xm_context_set_collapse: this context aligns one query of each group of byte-identical queries of a batch and copies its results to the
        others (AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291, within a batch).  Same results; the work counters then count the queries
        aligned, and BatchResult.copies the ones served as copies.  Off by default."""
        _check(self._L.xm_context_set_collapse(self._h, 1 if enable else 0))

    def set_memo(self, max_bytes):
        """xm_context_set_memo: this context remembers the queries it aligns in up to max_bytes of HBM and serves byte-identical queries of later batches from
        there (the run-wide AlignmentCache of AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291); it implies set_collapse within a batch.  Same
        results; BatchResult.remembered counts the queries served.  0 switches it off and frees it.  Off by default."""
        _check(self._L.xm_context_set_memo(self._h, int(max_bytes)))

    def memo_info(self):
        """xm_context_memo_info -> {entries, bytes_used, capacity, times_emptied}."""
        out = (C.c_int64 * 4)()
        _check(self._L.xm_context_memo_info(self._h, out))
        return {"entries": out[0], "bytes_used": out[1], "capacity": out[2], "times_emptied": out[3]}

    def attach_memory(self, memory):
        """xm_context_attach_memory: this context looks its queries up in `memory` (a QueryMemory of this index on this GPU, shared with the other contexts
        attached to it) and remembers what it aligns there; None detaches.  Same results; BatchResult.remembered counts the queries served."""
        if memory is not None and not getattr(memory, "_h", None):
            raise ValueError("the QueryMemory is closed")
        _check(self._L.xm_context_attach_memory(self._h, memory._h if memory is not None else None))

    def close(self):
        if getattr(self, "_h", None):
            self._L.xm_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def info(self):
        i = _capi.XmIndexInfo()
        _check(self._L.xm_index_get_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in _capi.XmIndexInfo._fields_}

    def ensure_length(self, n):
        _check(self._L.xm_index_ensure_length(self._h, int(n)))

    def table_shape(self, used_length):
        """(capacity, per-key limit) of the table of one gapmer length."""
        cap, mx = C.c_int32(), C.c_int32()
        _check(self._L.xm_index_table_shape(self._h, int(used_length), C.byref(cap), C.byref(mx)))
        return cap.value, mx.value

    def table(self, used_length):
        cap, mx, n, o = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        if self._L.xm_index_table_info(self._h, used_length, C.byref(cap), C.byref(mx), C.byref(n), C.byref(o)):
            return None
        counts = np.zeros(cap.value, dtype=np.int32)
        pos = np.zeros(max(n.value, 1), dtype=np.int64)
        self._L.xm_index_table_dump(self._h, used_length, counts.ctypes.data, pos.ctypes.data)
        return dict(capacity=cap.value, maxCount=mx.value, counts=counts, positions=pos[:n.value])

    def bucket_stats(self):
        """{buckets, occupied, overfull} over all hashed tables (overfull: more than max(L^2, 5) entries, HashBlock_Database.java:569-577)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._L.xm_index_bucket_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"buckets": a.value, "occupied": b.value, "overfull": c.value, "overfull_share_of_occupied": round(c.value / max(1, b.value + c.value), 6)}

    def dup_keys(self, contig):
        n = self._L.xm_index_dup_keys(self._h, contig, None, 0)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self._L.xm_index_dup_keys(self._h, contig, out.ctypes.data, n)
        return out[:n]

    def align_arrays(self, mate_count, mate_offset, mate_length, codes, expected_inner, deviation, parameters):
        """One AlignerWorker.process() batch (AlignerWorker.java:177-231) from flat arrays -> BatchResult."""
        b, keep = _capi.make_batch(mate_count, mate_offset, mate_length, codes, expected_inner, deviation)
        return self._align(lambda p, res: self._L.xm_align_batch(self._h, p, C.byref(b), res), parameters)

    def _align(self, call, parameters):
        """call(address of the xm_params, address of the result pointer) is the C entry that aligns -> BatchResult over its streams."""
        p = parameters._c() if isinstance(parameters, AlignmentParameters) else parameters
        res = C.POINTER(_capi.XmResult)()
        _check(call(C.byref(p), C.byref(res)), "Failed to align: ")
        return BatchResult(_capi.view_result(self._L, res))

    def upload_arrays(self, mate_count, mate_offset, mate_length, codes, expected_inner, deviation):
        """xm_batch_upload: validate + copy one batch to HBM; it stays resident for align_resident()."""
        b, keep = _capi.make_batch(mate_count, mate_offset, mate_length, codes, expected_inner, deviation)
        _check(self._L.xm_batch_upload(self._h, C.byref(b)))

    def stage_arrays(self, mate_count, mate_offset, mate_length, codes, expected_inner, deviation):
        """xm_batch_stage: copy the NEXT batch to HBM on its own stream (may run while align_resident() works on the resident batch)."""
        b, keep = _capi.make_batch(mate_count, mate_offset, mate_length, codes, expected_inner, deviation)
        _check(self._L.xm_batch_stage(self._h, C.byref(b)))

    def stage_fastq(self, block):
        """xm_batch_stage_fastq: the NEXT batch from FASTQ text (a hostio.TextBlock) - the text is copied to HBM and parsed there by kernels; the block then
        offers the arrays hostio.Batch offers (names and qualities included, for the writers).  A text that is not of the strict form (four lines a record, '@'
        headers, 1 .. 30000 bases) is a hostio.StrictFormError (a ValueError) that names file, record and reason, and nothing is staged.  A block cut with a
        split size (hostio.read_text_blocks(split=...)) is staged with it: the kernels cut every record into its sections, each a query, and a record may be
        longer than 30000 bases; a query count that is not the cutter's is an internal error.  A block of FASTA text (hostio.read_text_blocks(fasta=True)) goes to
        xm_batch_stage_fasta with its line counts: records of any number of lines, the same arrays, no qualities."""
        if block._text is None:
            raise ValueError("the block's text is gone: it has been staged or closed")
        t = block._text.contents
        out = C.POINTER(_capi.XmFastqBatch)()
        keep = 1 if block.keep_qualities else 0
        if block.fasta:
            text = _capi.XmFastaText(t.text1, t.bytes1, t.records1, t.lines1, t.text2, t.bytes2, t.records2, t.lines2, block.pair_spacing[0], block.pair_spacing[1], keep, block.split)
            rc = self._L.xm_batch_stage_fasta(self._h, C.byref(text), C.byref(out))
        else:
            text = _capi.XmFastqText(t.text1, t.bytes1, t.records1, t.text2, t.bytes2, t.records2, block.pair_spacing[0], block.pair_spacing[1], keep, block.split)
            rc = self._L.xm_batch_stage_fastq(self._h, C.byref(text), C.byref(out))
        if rc:
            raise hostio.StrictFormError(self._L.xm_last_error().decode())
        if int(out.contents.num_queries) != block.num_queries:  # (the cutter and the kernels count a split block's sections by the same rule)
            n = int(out.contents.num_queries)
            self._L.xm_fastq_batch_free(out)
            self._L.xm_batch_unstage(self._h)
            raise RuntimeError("%s: internal: the kernels built %d queries of a block the cutter counted %d in" % ("xm_batch_stage_fasta" if block.fasta else "xm_batch_stage_fastq", n, block.num_queries))
        block.attach(out, self._L.xm_fastq_batch_free)
        return block

    def set_sam_contigs(self, names):
        """xm_sam_set_contigs: the contig names of the SAM records format_sam_last builds (RNAME, RNEXT), one per contig of the index in its order; once per context."""
        arr = (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
        _check(self._L.xm_sam_set_contigs(self._h, len(names), arr))

    def format_sam_last(self, batch=None):
        """xm_sam_format_last: the SAM records of the last align call, formatted on the GPU from the result streams and the batch where they lie in HBM, while
        the batch is still resident (align_stream's on_aligned hook is the place) -> SamText.  batch: where the mates' names come from - None: the names that
        stage_fastq built, which are in HBM with the batch; else a hostio.Batch (or anything whose _ptr is a hostio.XmioBatch), whose names are copied up.
        The bytes equal hostio.Writer's for the same batch and streams."""
        t0 = time.perf_counter()
        out = C.POINTER(_capi.XmSamText)()
        names = None
        if batch is not None:
            raw = batch._ptr.contents
            names = _capi.XmSamNames(raw.names, C.cast(raw.name_off, C.c_void_p))
        _check(self._L.xm_sam_format_last(self._h, C.byref(names) if names is not None else None, C.byref(out)))
        self._tick("format", time.perf_counter() - t0)
        return SamText(self._L, out)

    def set_result_copy(self, on):
        """xm_context_set_result_copy: on=False - every later align call of this context leaves its four result streams in HBM and copies none of them to the
        host; the BatchResult then has ints = dbls = int_off = dbl_off = None (len(), num_ints, num_dbls, the counters and the times are what they are with the
        copy), and format_sam_last, summary_last and the pile-up read the streams where they lie.  True (the default) brings the copy back."""
        _check(self._L.xm_context_set_result_copy(self._h, 1 if on else 0))

    def summary_last(self, want_unaligned=False):
        """xm_summary_last: the statistics of the last align call's result streams, its alignments' penalties and (want_unaligned) its unaligned queries,
        computed on the GPU while the batch is still resident (align_stream's on_aligned hook is the place) -> BatchSummary.  hostio.Writer.write(batch, result,
        summary=...) makes of it what it makes of the streams."""
        t0 = time.perf_counter()
        out = C.POINTER(_capi.XmBatchSummary)()
        _check(self._L.xm_summary_last(self._h, 1 if want_unaligned else 0, C.byref(out)))
        self._tick("format", time.perf_counter() - t0)
        return BatchSummary(self._L, out)

    def unaligned_format_last(self):
        """xm_unaligned_format_last: the unaligned-query file's text of the last align call - every query without an alignment as it came in, FASTQ where it
        came with qualities, else FASTA - made on the GPU from the batch and the result streams where they lie in HBM, while the batch is still resident
        (align_stream's on_aligned hook is the place) -> SamText, whose `records` counts the mates written.  The batch must have been staged from text
        (stage_fastq): a batch staged from arrays has no names in HBM.  The bytes equal hostio.Writer's for the same batch and streams;
        hostio.Writer.write(batch, result, summary=..., unaligned_text=...) writes them."""
        t0 = time.perf_counter()
        out = C.POINTER(_capi.XmSamText)()
        _check(self._L.xm_unaligned_format_last(self._h, C.byref(out)))
        self._tick("format", time.perf_counter() - t0)
        return SamText(self._L, out)

    def set_batch_copy(self, on):
        """xm_context_set_batch_copy: on=False - every later stage_fastq of this context leaves the batch it builds in HBM and copies down only the mate counts,
        offsets and lengths; the block then has codes = None, block[k] raises, and its _ptr holds no names, codes or qualities.  format_sam_last(None),
        summary_last, unaligned_format_last and the pile-up read the batch where it lies.  True (the default) brings the copy back."""
        _check(self._L.xm_context_set_batch_copy(self._h, 1 if on else 0))

    def refs_count_last(self, raw=False):
        """xm_refs_count_last: the queries of the last align call counted per combination of contigs - for every query with an alignment the set of contigs
        its alignments lie on - on the GPU while the batch is still resident (align_stream's on_aligned hook is the place), with or without the copy of the
        streams -> {tuple of ascending contig indices: queries}; raw=True: the RefsCount it is folded from."""
        t0 = time.perf_counter()
        out = C.POINTER(_capi.XmRefsCount)()
        _check(self._L.xm_refs_count_last(self._h, C.byref(out)))
        got = RefsCount(self._L, out)
        self._tick("format", time.perf_counter() - t0)
        return got if raw else got.counts()

    def commit_staged(self):
        """xm_batch_commit: the staged batch becomes the resident one."""
        _check(self._L.xm_batch_commit(self._h))

    def unstage(self):
        """xm_batch_unstage: a staged batch that will not be committed is dropped (none staged: nothing happens)."""
        _check(self._L.xm_batch_unstage(self._h))

    def align_stream(self, batches, parameters, on_aligned=None):
        """Aligns a sequence of batches (each a tuple of upload_arrays' six arrays, or a hostio.TextBlock, which is staged with stage_fastq) and yields their BatchResults in order.  The copy of
        batch k+1 to HBM runs on a second host thread and a second stream while batch k is being aligned (the
        reference's workers fetch their next batch the same way, AlignerWorker.java:92-175)."""
        import queue
        import threading
        ready = queue.Queue()
        aligned = threading.Semaphore(0)
        stop = threading.Event()

        def uploader():
            try:
                first = True
                for arrays in batches:
                    if stop.is_set():
                        break
                    t0 = time.perf_counter()
                    if isinstance(arrays, hostio.TextBlock):  # FASTQ text: parsed on the GPU
                        self.stage_fastq(arrays)
                    else:
                        self.stage_arrays(*arrays)
                    self._tick("stage", time.perf_counter() - t0)
                    if not first:
                        aligned.acquire()  # the previous batch has been aligned: its buffers may be swapped away
                        if stop.is_set():
                            break
                    self.commit_staged()
                    first = False
                    ready.put(True)
                ready.put(None)
            except BaseException as e:  # noqa: BLE001  (handed to the consumer)
                ready.put(e)

        t = threading.Thread(target=uploader, daemon=True)
        t.start()
        count = 0
        try:
            while True:
                token = ready.get()
                if token is None:
                    break
                if isinstance(token, BaseException):
                    raise token
                t0 = time.perf_counter()
                r = self.align_resident(parameters)
                self._tick("align", time.perf_counter() - t0)
                if on_aligned is not None:  # (while the batch and its result streams are still resident: pileup.MatchDatabase.add_last)
                    on_aligned(count)
                count += 1
                aligned.release()
                yield r
        finally:
            stop.set()
            aligned.release()
            t.join(timeout=60)
            if not t.is_alive():  # (a stream that ends early - an align call failed, the caller went away - leaves no batch staged behind it)
                self.unstage()

    def align_resident(self, parameters):
        return self._align(lambda p, res: self._L.xm_align_resident(self._h, p, res), parameters)

    @staticmethod
    def batch_arrays(queries):
        """The six arrays of upload_arrays / align_arrays for a list of Query objects."""
        nq = len(queries)
        mc = np.zeros(nq, np.int32); mo = np.zeros(2 * nq, np.int64); ml = np.zeros(2 * nq, np.int32)
        ei = np.zeros(nq); dv = np.ones(nq)
        chunks, off = [], 0
        for i, q in enumerate(queries):
            mc[i] = len(q.sequences)
            ei[i], dv[i] = q.expected_inner_distance, q.spacing_deviation_per_unit_penalty
            for m, s in enumerate(q.sequences):
                mo[2 * i + m], ml[2 * i + m] = off, len(s)
                chunks.append(s)
                off += len(s)
        codes = np.concatenate(chunks) if chunks else np.zeros(1, np.uint8)
        return mc, mo, ml, codes, ei, dv

    def align_batches(self, queries, parameters, batch_size, on_aligned=None):
        """Aligns `queries` in batches of `batch_size` (AlignerWorker takes its queries batch by batch too, AlignerWorker.java:92-231) and
        yields (first query index, BatchResult) per batch; the next batch is packed and copied to HBM while the current one is aligned
        (align_stream).  on_aligned(replica, first query index, queries of the batch) is called while the batch is still resident."""
        starts = list(range(0, len(queries), max(1, int(batch_size))))
        arrays = (self.batch_arrays(queries[s:s + batch_size]) for s in starts)
        hook = (lambda k: on_aligned(0, starts[k], queries[starts[k]:starts[k] + batch_size])) if on_aligned else None
        for s, r in zip(starts, self.align_stream(arrays, parameters, on_aligned=hook)):
            yield s, r

    def align_batch(self, queries, parameters):
        return self.align_arrays(*self.batch_arrays(queries), parameters)

    def seed_probe(self, used_length, keys, max_per_probe=8, unpack=True):
        """Bulk PackedMap.get (PackedMap.java:160-172) on the device -> (counts, positions[n, max_per_probe] with -1 behind a probe's positions, kernel_ms).
        max_per_probe: 0 ... 15 (a bucket line holds seven; xm_seed_probe_packed refuses more than 15).  The C entry packs the positions of every 64 consecutive
        probes one behind the other: unpacked here.  unpack=False: (counts, None, kernel_ms) - the kernel fetches the positions all the same (that is what a
        measurement times), but they are not copied back to the host (n * max_per_probe * 8 bytes: 3.6 GB for 64 M probes with seven positions)."""
        used = np.ascontiguousarray(used_length, dtype=np.int32)
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        n = len(used)
        counts = np.zeros(n, np.int32)
        packed = np.zeros(max(max_per_probe, 1) * max(n, 1), np.int64) if unpack else None
        ms = C.c_double()
        _check(self._L.xm_seed_probe_packed(self._h, n, used.ctypes.data, keys.ctypes.data, max_per_probe, counts.ctypes.data, packed.ctypes.data if unpack else None, C.byref(ms)))
        if not unpack:
            return counts, packed, ms.value
        pos = np.full((n, max(max_per_probe, 1)), -1, np.int64)
        if max_per_probe > 0 and n > 0:
            m = np.minimum(np.maximum(counts, 0), max_per_probe).astype(np.int64)
            chunk = np.arange(n, dtype=np.int64) // 64
            run = np.cumsum(m) - m                                    # exclusive running sum over all probes ...
            start = run - run[chunk * 64] + chunk * 64 * max_per_probe  # ... made relative to the probe's chunk
            for j in range(max_per_probe):
                sel = m > j
                pos[sel, j] = packed[start[sel] + j]
        return counts, pos, ms.value


class QueryMemory:
    """xm_memory_new: one memory of aligned queries on the GPU of `db`, for any number of contexts of that index on that GPU (ReferenceDatabase.attach_memory):
    the reference's AlignmentCache is one map for the run that every AlignerWorker reads and fills (Api.java:62,82).  Two generations keep it remembering
    however long the run is: when the young one is full they turn - the old one is dropped, the young becomes the old - and a query served from the old one
    is copied into the young one (a second chance), so queries that keep coming back stay.  generations=1: full means nothing more is remembered.
    The memory lives until it is closed and its last context has detached or been closed, in any order."""
    FIELDS = ("entries", "bytes_used", "capacity", "times_emptied", "turns", "promoted", "contexts", "generations")

    def __init__(self, db, max_bytes, generations=2):
        self._L = _capi.lib()
        h = C.c_void_p()
        _check(self._L.xm_memory_new(db._h, int(max_bytes), int(generations), C.byref(h)))
        self._h = h

    def info(self):
        """xm_memory_info -> {entries, bytes_used, capacity, times_emptied, turns, promoted, contexts, generations}."""
        out = (C.c_int64 * 8)()
        _check(self._L.xm_memory_info(self._h, out))
        return dict(zip(self.FIELDS, (int(x) for x in out)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.xm_memory_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def measure_random_gather(table_bytes=4 << 30, accesses=1 << 26, device=0):
    """Random 64-byte-sector reads per second the GPU sustains (xm_measure_random_gather) -> (sectors/s, kernel ms)."""
    L = _capi.lib()
    ms = C.c_double()
    _check(L.xm_measure_random_gather(device, table_bytes, accesses, C.byref(ms)))
    return accesses / (ms.value * 1e-3), ms.value


def device_memory(device=0):
    """xm_device_memory: (free, total) bytes of HBM on GPU `device` right now."""
    L = _capi.lib()
    f, t = C.c_int64(), C.c_int64()
    _check(L.xm_device_memory(int(device), C.byref(f), C.byref(t)))
    return f.value, t.value


def divide_scratch(contexts, device, reserve=24 << 30, most=200 << 30, per_context_extra=0, shared_extra=0):
    """Several contexts on one GPU: what is free now (the index is resident) minus a reserve for batches and result arenas and minus what every
    context will allocate beside its scratch (per_context_extra: a pile-up of 40-48 bytes per reference base with --out-mutations), in equal
    parts; a context that would get less than 8 GiB is not worth having -> (how many of `contexts` to use, bytes each).  shared_extra: what will be
    allocated on this GPU once, however many contexts it has (the GPU's QueryMemory)."""
    for c in contexts:
        c.set_scratch(1 << 20)  # (a context that already holds scratch gives it back first: what is free is then what there is to divide)
    free, _ = device_memory(device)
    reserve = min(int(reserve), int(free) // 4)  # (a small or busy GPU: the reserve is a share of what there is, not a fixed claim)
    free -= int(shared_extra)
    n = len(contexts)
    while n > 1 and (free - reserve - n * per_context_extra) // n < (8 << 30):
        n -= 1
    share = max(256 << 20, min(most, (free - reserve - n * per_context_extra) // max(n, 1)))
    for c in contexts[:n]:
        c.set_scratch(share)
    for c in contexts[n:]:
        c.set_scratch(0)
    return n, share


def sort_reference(contigs):
    """Mapper.sortAndComplementReference (Mapper.java:1151-1172): length-descending, stable within equal lengths."""
    return sorted(contigs, key=lambda c: -len(c[1]))


# ---- Api.java:18-107
def newDatabase(references, **kw):
    """Api.newDatabase(List<String>) (Api.java:25-31): contigs are named reference-<i>."""
    if isinstance(references, str):
        references = [references]
    if isinstance(references, dict):
        items = list(references.items())
    else:
        items = [("reference-%d" % i, r) for i, r in enumerate(references)]
    kw.setdefault("mode", "api")
    return ReferenceDatabase(items, **kw)


def align(query, reference_database, parameters):
    """Api.align (Api.java:79-92) -> List<QueryAlignment> (QueryAlignments.getTopLevelAlignments())."""
    if isinstance(query, str):
        query = Query(query)
    comps = reference_database.align_batch([query], parameters).query_alignments(0)
    return comps[0] if len(comps) == 1 else []


def alignOnce(query, reference_text, parameters):
    """Api.alignOnce (Api.java:96-107)."""
    db = newDatabase(reference_text)
    try:
        return align(query, db, parameters)
    finally:
        db.close()
