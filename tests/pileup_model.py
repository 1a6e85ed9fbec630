"""A plain recount of the pile-up (xm_pileup_* of include/xmapper_hip.h), written from the documented rules and not from the kernel.

TEST INFRASTRUCTURE ONLY.  The model takes the decoded alignments of a batch (api.decode_streams / BatchResult.query_alignments: per query a list of
components, each a list of QueryAlignment), the batch's mates, the contigs and a query-end fraction, and keeps per contig `depth`, `alt[4]` and
`middle` as exact integers in units of 1 / UNIT (uint64; no float is ever added), plus the events with all eight fields.  The rules:

* a component with n >= 1 alignments gives alignment a (0-based, stream order) the weight UNIT // n + (1 if a < UNIT % n else 0);
* every reference base under an equal-length block and every base of a deletion block (lengthA == 0) gets the weight in `depth`;
* under an equal-length block the query base is the mate's base at startA + i on the strand that was aligned; it is counted in alt[A|C|G|T] only
  when it and the reference base are both unambiguous and differ;
* one component: sequence k of an alignment is mate k; two components (the pair fell back to unpaired alignments): component c is mate c;
* two sequence alignments of one pair alignment on the same contig share the depth where their reference intervals intersect: there the first
  adds w // 2 and the second w - w // 2 (depth, alt, middle and event weight - an event's weight is that of a base at its startB);
* near a query end: k < f * len or k >= len - f * len in doubles, len the mate's own length, k the index on the aligned strand; a deletion's bases
  take k = startA of the block; an event carries flag bit 2 by the same test at startA, only when f > 0; with f == 0 the middle depth is the depth;
* one event per block with lengthA != lengthB: (contig, startB, 1 insertion / 2 deletion, length, query ordinal over all batches added,
  mate | reversed << 1 | near_end << 2, startA, weight).

Every add() asserts conservation on its own output: the weights of a query's alignments sum to UNIT per non-empty component, and the depth added
over all contigs equals the model's own count of weight x reference bases covered."""
import numpy as np

UNIT = 1441440  # XM_PILEUP_UNIT (include/xmapper_hip.h)

_COMPLEMENT = np.array([((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3) for b in range(16)], dtype=np.uint8)
_PLANE = np.full(16, -1, dtype=np.int64)  # unambiguous code -> alt plane
_PLANE[[1, 2, 4, 8]] = [0, 1, 2, 3]


def alignment_weights(n):
    """The n weights of a component with n alignments, in stream order."""
    return [UNIT // n + (1 if a < UNIT % n else 0) for a in range(n)]


def near_query_end(k, length, f):
    """k (an int or an int array) lies within the fraction f of `length` of either query end - in doubles, exactly as documented."""
    k = np.asarray(k, dtype=np.float64)
    return (k < f * length) | (k >= length - f * length)


def event_order(e):
    """The order xm_pileup_add_last documents for the events of a call: (ordinal, contig, position, flags, startA)."""
    return (e[4], e[0], e[1], e[5], e[6])


class PileupModel:
    def __init__(self, contigs, query_end_fraction=0.0):
        """contigs: list of (name, code array)."""
        self.contigs = [(n, np.asarray(c, dtype=np.uint8)) for n, c in contigs]
        self.f = float(query_end_fraction)
        self.depth = [np.zeros(len(c), np.uint64) for _, c in self.contigs]
        self.alt = [np.zeros((4, len(c)), np.uint64) for _, c in self.contigs]
        self.middle = [np.zeros(len(c), np.uint64) for _, c in self.contigs]
        self.events = []
        self.queries_added = 0
        self.covered = 0  # sum over every block added of weight x reference bases (a Python int)

    def _block_weights(self, start_b, n, w, share, overlap):
        """The weight of each of the n reference bases from start_b: w, and `share` inside the overlap (lo, hi) with the other mate."""
        wv = np.full(n, w, np.uint64)
        if overlap is not None:
            lo, hi = max(overlap[0], start_b), min(overlap[1], start_b + n)
            if lo < hi:
                wv[lo - start_b:hi - start_b] = share
        return wv

    def add(self, alignments, mates):
        """One batch: alignments[q] = decoded components of query q, mates[q] = its 1 or 2 code arrays.  Returns the running number of events."""
        assert len(alignments) == len(mates)
        f = self.f
        depth_before = sum(int(d.sum(dtype=np.uint64)) for d in self.depth)
        covered_before = self.covered
        for q, comps in enumerate(alignments):
            for c, als in enumerate(comps):
                if not als:
                    continue
                weights = alignment_weights(len(als))
                assert sum(weights) == UNIT and max(weights) - min(weights) <= 1
                for al, w in zip(als, weights):
                    seqs = al.components
                    overlap = None
                    if len(seqs) == 2 and seqs[0].contig == seqs[1].contig and seqs[0].sections and seqs[1].sections:
                        lo = max(s.start_index_b() for s in seqs)
                        hi = min(s.end_index_b() for s in seqs)
                        if lo < hi:
                            overlap = (lo, hi)
                    for k, sa in enumerate(seqs):
                        mate = c if len(comps) > 1 else k
                        read = np.asarray(mates[q][mate], dtype=np.uint8)
                        oriented = _COMPLEMENT[read[::-1]] if sa.reference_reversed else read
                        share = w // 2 if k == 0 else w - w // 2
                        ref = self.contigs[sa.contig][1]
                        depth, alt, middle = self.depth[sa.contig], self.alt[sa.contig], self.middle[sa.contig]
                        for b in sa.sections:
                            if b.lengthA == b.lengthB:
                                n = b.lengthB
                                wv = self._block_weights(b.startB, n, w, share, overlap)
                                np.add.at(depth, slice(b.startB, b.startB + n), wv)
                                inner = ~near_query_end(np.arange(b.startA, b.startA + n), len(read), f)
                                np.add.at(middle, b.startB + np.nonzero(inner)[0], wv[inner])
                                qb, rb = oriented[b.startA:b.startA + n], ref[b.startB:b.startB + n]
                                differs = (_PLANE[qb] >= 0) & (_PLANE[rb] >= 0) & (qb != rb)
                                at = np.nonzero(differs)[0]
                                np.add.at(alt, (_PLANE[qb[at]], b.startB + at), wv[at])
                                self.covered += int(wv.sum(dtype=np.uint64))
                                continue
                            near = bool(near_query_end(b.startA, len(read), f))
                            if b.lengthA == 0:
                                n = b.lengthB
                                wv = self._block_weights(b.startB, n, w, share, overlap)
                                np.add.at(depth, slice(b.startB, b.startB + n), wv)
                                if not near:
                                    np.add.at(middle, slice(b.startB, b.startB + n), wv)
                                self.covered += int(wv.sum(dtype=np.uint64))
                            here = share if overlap is not None and overlap[0] <= b.startB < overlap[1] else w
                            flags = mate | (int(sa.reference_reversed) << 1) | (4 if f > 0 and near else 0)
                            self.events.append((sa.contig, b.startB, 1 if b.lengthA > 0 else 2, b.lengthA if b.lengthA > 0 else b.lengthB,
                                                self.queries_added + q, flags, b.startA, here))
        self.queries_added += len(alignments)
        added = sum(int(d.sum(dtype=np.uint64)) for d in self.depth) - depth_before
        assert added == self.covered - covered_before, "the depth added (%d) is not weight x bases covered (%d)" % (added, self.covered - covered_before)
        for c in range(len(self.contigs)):
            assert np.all(self.middle[c] <= self.depth[c]) and np.all(self.alt[c].sum(axis=0) <= self.depth[c])
            if f == 0:
                assert np.array_equal(self.middle[c], self.depth[c])
        return len(self.events)

    def sorted_events(self):
        return sorted(self.events, key=event_order)
