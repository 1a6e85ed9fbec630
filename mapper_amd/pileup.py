"""Pile-up of alignments on the reference and the mutations file.

Mapper.run hands every batch of QueryAlignments to a MatchDatabase (Mapper.java:700-708) and, when the run is over, writes
`--out-mutations` / `--out-vcf` from MatchDatabase.groupByPosition() (Mapper.java:758-785).  MatchDatabase, Alignments, AlignmentPosition,
MutationsWriter and MutationDetectionParameters live in the un-vendored QuickVariants module; what this file reproduces is what the
reference's own tests pin: src/test/java/MatchDatabase_Test.java:12-69 (every aligned reference base counts 1; the two mates of a pair count
1 together where they overlap) and src/test/java/MutationsWriter_Test.java:18-134 (the line format `contig, 1-based position, reference
allele, query allele, allele depth, total depth`; a deletion is reported at its first base with the deleted bases against dashes, an insertion
at the base before it with dashes against the inserted bases; consecutive substitutions are separate lines; the total-depth filter).
--distinguish-query-ends (MatchDatabase(queryEndFraction), Mapper.java:76,351-353,700): "when detecting indels, only consider the middle of each query"
(Mapper.java:532) - the indel thresholds look at the *middle* depth, the depth from query bases that are not within the fraction of the query's
length of either query end (Mapper.java:538-542 "total (middle) depth"), and an indel near a query end does not support itself; pinned by
MutationsWriter_Test.java:114-134 (fraction 0.5 = every base is near an end: the insertion is not reported once a middle depth of 1 is asked for).
[unpinned]: the header lines (the reference's test strips lines that start with '#' or 'CHR'), the weight of a query with several
alignments (taken as 1/n each), how ambiguous bases count (depth only), the order of lines at one position, where exactly "near the end" stops
(here: query index k with k < f * length or k >= length - f * length), the supporting-depth fractions and the continuation thresholds
(Mapper.java:208-230: taken as alt / total; an indel is cut where its continuation fails).

The accumulation itself runs on the GPU (xm_pileup_kernel: one lane per query walks its result stream in HBM and adds to per-position
integer counters, so the result does not depend on the order of the atomic adds); this module holds the host side.  The bases of an insertion come
from the queries handed to add_last or, with keep_insert_text, from the device pile-up, which then keeps them beside the event (xm_pileup_text.h):
a job that streams its batches needs no query after its batch is written."""
import ctypes as C
import heapq

import numpy as np

from . import _capi
from .api import decode, reverse_complement

UNIT = 1441440  # XM_PILEUP_UNIT (include/xmapper_hip.h)


class MutationDetectionParameters:
    """MutationDetectionParameters [QuickVariants]: the six thresholds Mapper.main fills in (Mapper.java:208-230).  emptyFilter() = everything is
    reported (what the reference's tests start from); defaultFilter() = the defaults --out-mutations documents (Mapper.java:534-542)."""

    def __init__(self, minSNPTotalDepth=0.0, minSNPDepthFraction=0.0, minIndelTotalStartDepth=0.0, minIndelStartDepthFraction=0.0,
                 minIndelContinuationTotalDepth=0.0, minIndelContinuationDepthFraction=0.0):
        # Mapper.main narrows every threshold to float - (float)Double.parseDouble(...), Mapper.java:203-230 - so they are kept as float32 values here and
        # the products with the depths are taken in float32 too (_below): 0.7 of a depth of 10 is 7.0 in float and 7.000000000000001 in double, and an
        # allele seen 7 times must not be dropped by the latter.  [inferred: the fields of MutationDetectionParameters live in QuickVariants]
        f32 = lambda x: float(np.float32(x))  # noqa: E731
        self.minSNPTotalDepth, self.minSNPDepthFraction = f32(minSNPTotalDepth), f32(minSNPDepthFraction)
        self.minIndelTotalStartDepth, self.minIndelStartDepthFraction = f32(minIndelTotalStartDepth), f32(minIndelStartDepthFraction)
        self.minIndelContinuationTotalDepth, self.minIndelContinuationDepthFraction = f32(minIndelContinuationTotalDepth), f32(minIndelContinuationDepthFraction)

    @staticmethod
    def emptyFilter():
        return MutationDetectionParameters()

    @staticmethod
    def defaultFilter():
        return MutationDetectionParameters(5.0, 0.9, 1.0, 0.8, 1.0, 0.7)


def _below(support, fraction, total):
    """support < fraction * total in float arithmetic (the thresholds are floats in the reference: Mapper.java:203-230)."""
    return bool(np.float32(support) < np.float32(fraction) * np.float32(total))


def _number(x):
    """Depths are sums of 1/n: whole numbers print without a fraction (MutationsWriter_Test: `1`), others like a Java float."""
    return str(int(x)) if float(x).is_integer() else repr(float(np.float32(x)))


class MatchDatabase:
    """MatchDatabase(queryEndFraction) + groupByPosition() for one ReferenceDatabase (or the replicas of a MultiGpuDatabase: one device pile-up
    each, summed on the host in replica order).  keep_insert_text: the device pile-ups keep the bases of every insertion with its event
    (xm_pileup_keep_insert_text), so add_last needs no queries for the text of insertions and nothing of a batch has to outlive it.  group_on_gpu: the
    device pile-ups group the insertion / deletion events themselves as the batches come in (xm_pileup_group_events): no event and no letter is
    copied to the host but the left-overs of fingerprint collisions, _indels() reads the groups, and mutations(on_gpu=True) has them judged where they lie."""

    group_on_gpu = False   # (subclasses that hold handed-in counts never group on a device)

    def __init__(self, databases, query_end_fraction=0.0, keep_insert_text=False, group_on_gpu=False):
        self.dbs = list(databases) if isinstance(databases, (list, tuple)) else [databases]
        self.query_end_fraction = float(query_end_fraction)
        self.group_on_gpu = bool(group_on_gpu)
        self.keep_insert_text = bool(keep_insert_text) or self.group_on_gpu   # (grouping needs the letters: the device keeps them)
        self._L = _capi.lib()
        self._h = []
        for db in self.dbs:
            h = C.c_void_p()
            if self._L.xm_pileup_new(db._h, C.byref(h)):
                raise RuntimeError(self._L.xm_last_error().decode())
            self._h.append(h)
            if self._L.xm_pileup_set_query_ends(h, self.query_end_fraction):
                raise RuntimeError(self._L.xm_last_error().decode())
            if self.keep_insert_text and self._L.xm_pileup_keep_insert_text(h, 1):
                raise RuntimeError(self._L.xm_last_error().decode())
            if self.group_on_gpu and self._L.xm_pileup_group_events(h, 1):
                raise RuntimeError(self._L.xm_last_error().decode())
        self.contigs = self.dbs[0].contigs
        self._reads = {}   # query ordinal (per replica) -> mates, kept only for queries with an insertion
        self._batches = [[] for _ in self.dbs]

    def add_last(self, queries=None, replica=0):
        """addAlignments(List<QueryAlignments>) for the batch replica `replica` aligned last (its streams are still in HBM).  `queries`: the
        batch's Query objects or mate arrays, needed for the text of insertions (None: the text the device kept, with keep_insert_text; without it
        insertions are reported by length only)."""
        if self.group_on_gpu and queries is not None:
            raise RuntimeError("add_last(queries) with group_on_gpu: the text of insertions is the device's, the events are grouped where they lie")
        n = C.c_int64(0)
        if self._L.xm_pileup_add_last(self._h[replica], C.byref(n)):
            raise RuntimeError(self._L.xm_last_error().decode())
        self._batches[replica].append(queries)
        return n.value

    def close(self):
        for h in self._h:
            self._L.xm_pileup_free(h)
        self._h = []

    def _sum(self, contig):
        n = len(self.contigs[contig][1])
        depth = np.zeros(n, np.uint64)
        alt = np.zeros((4, n), np.uint64)
        for h in self._h:  # fixed replica order (integer sums: any order gives the same, the order is kept for the record)
            d = np.zeros(n, np.uint64)
            a = np.zeros((4, n), np.uint64)
            if self._L.xm_pileup_read(h, contig, 0, n, d.ctypes.data, a.ctypes.data):
                raise RuntimeError(self._L.xm_last_error().decode())
            depth += d
            alt += a
        return depth, alt

    def depth(self, contig):
        """AlignmentPosition.getCount() for every position of the contig."""
        return self._sum(contig)[0].astype(np.float64) / UNIT

    def _middle(self, contig):
        """The depth from query bases away from the query ends (all of it without a query-end fraction), summed over the replicas."""
        n = len(self.contigs[contig][1])
        mid = np.zeros(n, np.uint64)
        for h in self._h:
            d = np.zeros(n, np.uint64)
            if self._L.xm_pileup_read_middle(h, contig, 0, n, d.ctypes.data):
                raise RuntimeError(self._L.xm_last_error().decode())
            mid += d
        return mid

    def _events(self):
        """(replica, contig, startB, type, length, query ordinal, mate | reversed << 1, startA, weight) of every insertion / deletion block.  With
        keep_insert_text the text is paged with the events: self._texts[(replica, k)] is the kept text of the replica's k-th event, for insertions."""
        out = []
        buf = np.zeros((1 << 16, 8), np.int64)
        self._texts = {}
        if self.keep_insert_text:
            off = np.zeros(len(buf) + 1, np.int64)
            text = np.zeros(1 << 20, np.uint8)
        for r, h in enumerate(self._h):
            first = 0
            while True:
                m = self._L.xm_pileup_events(h, first, len(buf), buf.ctypes.data)
                if m <= 0:
                    break
                if self.keep_insert_text:
                    # (a page of text may hold fewer events than asked for; an insertion longer than the page gets a page of its size)
                    while (got := self._L.xm_pileup_event_text(h, first, m, off.ctypes.data, text.ctypes.data, len(text))) < 0:
                        if len(text) >= 1 << 40:
                            raise RuntimeError("xm_pileup_event_text failed for event %d of replica %d" % (first, r))
                        text = np.zeros(2 * len(text), np.uint8)
                    m = got
                    for k in np.nonzero(buf[:m, 2] == 1)[0]:
                        self._texts[(r, first + int(k))] = text[off[k]:off[k + 1]].tobytes().decode("ascii")
                out += [(r,) + tuple(int(x) for x in row) for row in buf[:m]]
                first += m
        return out

    def _mate(self, replica, ordinal, mate):
        at = 0
        for qs in self._batches[replica]:
            if qs is None:
                return None
            if ordinal < at + len(qs):
                q = qs[ordinal - at]
                seqs = q.sequences if hasattr(q, "sequences") else q
                return np.asarray(seqs[mate], dtype=np.uint8)
            at += len(qs)
        return None

    def _device_groups(self, h, filt=None):
        """xm_pileup_call_indels of one device pile-up -> (xm_indel_call records, their letters, the call's figures); filt None: every group, unjudged."""
        calls = C.POINTER(_capi.XmIndelCalls)()
        if self._L.xm_pileup_call_indels(h, C.byref(filt) if filt is not None else None, C.byref(calls)):
            raise RuntimeError(self._L.xm_last_error().decode())
        try:
            return _capi.indel_calls(calls)
        finally:
            self._L.xm_indel_calls_free(calls)

    def _group_keys(self, rows, letters):
        """The keys of _indels() for xm_indel_call records: one Python object per record that came down, none per event."""
        keys = []
        for c, kind, pos1, length, at, n in zip(rows["contig"].tolist(), rows["kind"].tolist(), rows["pos1"].tolist(), rows["length"].tolist(), rows["letters_at"].tolist(),
                                                rows["num_letters"].tolist()):
            if kind == 1:
                keys.append((c, pos1, 1, "-" * length, letters[at:at + n].decode("ascii")))
            else:
                keys.append((c, pos1, 2, decode(self.contigs[c][1][pos1 - 1:pos1 - 1 + length]), "-" * length))
        return keys

    def _indels(self):
        """The insertion / deletion events away from the query ends, grouped: (contig, 1-based position, kind 1 insertion / 2 deletion, reference allele, query
        allele) -> summed weight in units, in the order the events first name them.  group_on_gpu: the groups of the device pile-ups in key order, and the
        groups of the left-over events behind them."""
        if self.group_on_gpu:
            indels = {}
            for h in self._h:
                rows, letters, _ = self._device_groups(h)
                for key, w in zip(self._group_keys(rows, letters), rows["support_units"].tolist()):
                    indels[key] = indels.get(key, 0) + w
            indels = dict(sorted(indels.items()))
            for key, w in self._host_indels().items():
                indels[key] = indels.get(key, 0) + w
            return indels
        return self._host_indels()

    def _host_indels(self):
        """_indels() over the events the host holds."""
        indels = {}
        events = self._events()
        kept = getattr(self, "_texts", {})
        seen = {}   # events of each replica so far: the index the kept text is filed under
        for r, contig, pos, kind, length, ordinal, flags, start_a, weight in events:
            at = seen[r] = seen.get(r, -1) + 1
            if flags & 4:   # near a query end: "when detecting indels, only consider the middle of each query" (Mapper.java:532)
                continue
            ref = self.contigs[contig][1]
            if kind == 1:
                mate = self._mate(r, ordinal, flags & 1)
                if mate is None:   # no queries were handed in for its batch: what the device kept, if it kept text
                    text = kept.get((r, at), "N" * length)
                else:
                    oriented = reverse_complement(mate) if (flags >> 1) & 1 else mate
                    text = decode(oriented[start_a:start_a + length])
                key = (contig, pos, 1, "-" * length, text)   # reported at the base before the insertion: 1-based position = startB
            else:
                key = (contig, pos + 1, 2, decode(ref[pos:pos + length]), "-" * length)
            indels[key] = indels.get(key, 0) + weight
        return indels

    def mutations(self, parameters=None, on_gpu=False):
        """-> list of (contig index, 1-based position, reference allele, query allele, allele depth, total depth), in contig and position order.
        on_gpu: the thresholds are applied where the counts lie (_mutations_on_gpu); the path below is the definition of what that returns."""
        f = parameters or MutationDetectionParameters.emptyFilter()
        if on_gpu:
            return self._mutations_on_gpu(f)
        rows = []
        indels = self._indels()
        for c in range(len(self.contigs)):
            depth, alt = self._sum(c)
            mid = self._middle(c) if indels else depth
            ref = self.contigs[c][1]
            for b, letter in enumerate("ACGT"):
                for pos in np.nonzero(alt[b])[0]:
                    total = depth[pos] / UNIT
                    support = alt[b][pos] / UNIT
                    if total < f.minSNPTotalDepth or _below(support, f.minSNPDepthFraction, total):
                        continue
                    rows.append((c, int(pos) + 1, 0, decode(ref[pos:pos + 1]), letter, support, total))
            for (cc, pos1, kind, ra, qa), w in indels.items():
                if cc != c:
                    continue
                support = w / UNIT
                at = min(max(pos1 - 1, 0), len(ref) - 1)
                total = mid[at] / UNIT     # the total (middle) depth where the indel starts (Mapper.java:538-539)
                if total < f.minIndelTotalStartDepth or _below(support, f.minIndelStartDepthFraction, total):
                    continue
                # continuation (Mapper.java:541-542) [inferred]: every further base of the indel is judged where it lies (a deletion's bases on the
                # reference, an insertion's at its one position); the indel is cut in front of the first base that fails
                n = max(len(ra), len(qa))
                keep = 1
                while keep < n:
                    here = min(at + keep, len(ref) - 1) if kind == 2 else at
                    t = mid[here] / UNIT
                    if t < f.minIndelContinuationTotalDepth or _below(support, f.minIndelContinuationDepthFraction, t):
                        break
                    keep += 1
                rows.append((c, pos1, kind, ra[:keep], qa[:keep], support, total))
        rows.sort(key=lambda t: (t[0], t[1], t[2], t[3], t[4]))
        return [(c, pos1, ra, qa, w, total) for c, pos1, _, ra, qa, w, total in rows]

    def _mutations_on_gpu(self, f):
        """mutations(f) without reading the pile-up back: every replica's counts are moved into the first pile-up (xm_pileup_absorb: the sums over
        the replicas stay what they were, so the host path still gives the same rows afterwards), the SNP rows come from the device in contig, position and
        letter order (xm_pileup_call_snps), and the indel candidates of all contigs - the events are host memory already and are grouped as ever - are judged
        in one call (xm_pileup_judge_indels).  What crosses to the host is the rows and a verdict per candidate.  self.last_on_gpu: the figures of the call.
        group_on_gpu: the absorb also moves the replicas' groups into the first pile-up's table, the groups are judged where they lie and only the
        kept ones come down (xm_pileup_call_indels); candidates are then the groups of the left-over events alone."""
        if not self._h:
            raise RuntimeError("mutations(on_gpu=True) needs a device pile-up")
        L, first = self._L, self._h[0]
        for h in self._h[1:]:
            if L.xm_pileup_absorb(first, h):
                raise RuntimeError(L.xm_last_error().decode())
        filt = _capi.XmMutationFilter(f.minSNPTotalDepth, f.minIndelTotalStartDepth, f.minIndelContinuationTotalDepth,
                                      f.minSNPDepthFraction, f.minIndelStartDepthFraction, f.minIndelContinuationDepthFraction, 0)
        calls = C.POINTER(_capi.XmSnpCalls)()
        if L.xm_pileup_call_snps(first, C.byref(filt), C.byref(calls)):
            raise RuntimeError(L.xm_last_error().decode())
        try:
            got = calls.contents
            n = int(got.num_rows)
            self.last_on_gpu = {"snp_rows": n, "bytes_to_host": int(got.bytes_to_host), "select_ms": got.kernel_ms, "d2h_ms": got.d2h_ms}
            snps = np.frombuffer((_capi.XmSnpRow * n).from_address(C.addressof(got.rows.contents)), dtype=_capi.SNP_ROW).copy() if n else np.zeros(0, _capi.SNP_ROW)
        finally:
            L.xm_snp_calls_free(calls)
        kept, kept_verdicts = [], np.zeros(0, _capi.INDEL_VERDICT)
        left = {}
        if self.group_on_gpu:
            left = self._host_indels()
        if self.group_on_gpu and not (left and len(self._h) > 1):
            # the groups are judged where they lie and only the kept ones come down; the left-overs' groups - disjoint from the table's - go the old way
            rows, letters, figures = self._device_groups(first, filt)
            kept = list(zip(self._group_keys(rows, letters), rows["support_units"].tolist()))
            kept_verdicts = np.zeros(len(rows), _capi.INDEL_VERDICT)
            kept_verdicts["total_units"], kept_verdicts["keep"] = rows["total_units"], rows["keep"]
            self.last_on_gpu.update(groups=figures["groups"], kept=len(rows), left_over=figures["left_over"], group_bytes_to_host=figures["bytes_to_host"],
                                    table_bytes=figures["table_bytes"], bytes_to_host=self.last_on_gpu["bytes_to_host"] + figures["bytes_to_host"])
            indels = list(left.items())
        else:
            # (left-overs of several pile-ups: a key may be left over in one and in the table of another, so the sums are made on the host before the judge)
            indels = list(self._indels().items())
        candidates = indel_candidates(indels)
        verdicts = np.zeros(len(indels), _capi.INDEL_VERDICT)
        if L.xm_pileup_judge_indels(first, C.byref(filt), candidates.ctypes.data, len(indels), verdicts.ctypes.data):
            raise RuntimeError(L.xm_last_error().decode())
        self.last_on_gpu.update(candidates=len(indels), bytes_to_host=self.last_on_gpu["bytes_to_host"] + verdicts.nbytes)
        return merged_rows(snps, kept + indels, np.concatenate([kept_verdicts, verdicts]), lambda contig, position, code: decode((code,)))

    def write_mutations(self, out, parameters=None, on_gpu=False):
        """MutationsWriter.write: one line per mutation.  The two header lines are [unpinned] (the reference's test drops '#' and 'CHR' lines)."""
        out.write("# mutations of the aligned queries against the reference\n")
        out.write("CHR\tPOS\tREF\tALT\tALT DEPTH\tTOTAL DEPTH\n")
        for c, pos1, ra, qa, w, total in self.mutations(parameters, on_gpu=on_gpu):
            out.write("%s\t%d\t%s\t%s\t%s\t%s\n" % (self.contigs[c][0], pos1, ra, qa, _number(w), _number(total)))


def indel_candidates(indels):
    """The groups of MatchDatabase._indels(), as a list of items -> xm_indel_candidate records, one per group in its order."""
    candidates = np.zeros(len(indels), _capi.INDEL_CANDIDATE)
    for i, ((c, pos1, kind, ra, qa), w) in enumerate(indels):
        candidates[i] = (c, kind, pos1, max(len(ra), len(qa)), w)
    return candidates


def merged_rows(snps, indels, verdicts, reference_allele):
    """The rows of mutations() from what the device (or the rules' test program) answered: snps, xm_snp_row records in contig, position and letter order;
    indels, the candidates' groups with verdicts, one xm_indel_verdict each.  reference_allele(contig, 0-based position, the row's reference code) -> text.
    The two sorted sets are merged by the key the host path sorts with."""
    rows = [(c, p + 1, 0, reference_allele(c, p, code), "ACGT"[b], s / UNIT, t / UNIT) for c, p, b, code, s, t in
            zip(snps["contig"].tolist(), snps["position"].tolist(), snps["letter"].tolist(), snps["reference_code"].tolist(), snps["support_units"], snps["total_units"])]
    judged = [(c, pos1, kind, ra[:keep], qa[:keep], w / UNIT, total / UNIT)
              for ((c, pos1, kind, ra, qa), w), total, keep in zip(indels, verdicts["total_units"], verdicts["keep"].tolist()) if keep > 0]
    key = lambda t: (t[0], t[1], t[2], t[3], t[4])  # noqa: E731
    judged.sort(key=key)
    return [(c, pos1, ra, qa, w, total) for c, pos1, _, ra, qa, w, total in heapq.merge(rows, judged, key=key)]


class CountedMatchDatabase(MatchDatabase):
    """The host half of MatchDatabase (event grouping, thresholds, continuation cut, line order) over counts that are handed in instead of read from
    a device pile-up: no library is loaded and no GPU is needed.  contigs: [(name, codes)]; depth[c], alt[c] ([4, n]) and middle[c] in units of 1 / UNIT;
    events: the eight fields of xm_pileup_events per event; batches: the queries of each batch added, in order (for the text of insertions)."""

    def __init__(self, contigs, depth, alt, middle, events, batches=(), query_end_fraction=0.0):
        self.dbs, self._h, self._L = [], [], None
        self.query_end_fraction = float(query_end_fraction)
        self.contigs = contigs
        self._counts = [(np.asarray(d, np.uint64), np.asarray(a, np.uint64), np.asarray(m, np.uint64)) for d, a, m in zip(depth, alt, middle)]
        self._event_rows = [(0,) + tuple(int(x) for x in e) for e in events]
        self._reads = {}
        self._batches = [list(batches)]

    def add_last(self, queries=None, replica=0):
        raise RuntimeError("CountedMatchDatabase holds counts that were handed in: there is no device batch to add")

    def _sum(self, contig):
        return self._counts[contig][0], self._counts[contig][1]

    def _middle(self, contig):
        return self._counts[contig][2]

    def _events(self):
        return list(self._event_rows)
