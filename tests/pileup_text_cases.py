"""Inputs of the insertion-text tests (tests/test_pileup_text_rules.py on the host, tests/test_gpu_pileup_text.py on the GPU) and the rule they compare with.

TEST INFRASTRUCTURE ONLY.  The rule is pileup.MatchDatabase.mutations' own: oriented = reverse_complement(mate) if reversed else mate;
text = decode(oriented[startA : startA + length]), through api.decode and api.reverse_complement.  Events are the eight fields of xm_pileup_events."""
import numpy as np

from mapper_amd import api


def synthetic_mates(nq, seed, lengths=(1, 2, 63, 64, 65, 150, 1200)):
    """nq pairs of mates of the given lengths (cycled, mate 2 one step further), every one of the 16 codes among the bases.
    -> (mate_offset[2 nq], mate_length[2 nq], codes)"""
    rng = np.random.default_rng(seed)
    mate_length = np.array([lengths[(q + m) % len(lengths)] for q in range(nq) for m in range(2)], np.int32)
    mate_offset = np.concatenate([[0], np.cumsum(mate_length[:-1])]).astype(np.int64)
    codes = rng.integers(0, 16, int(mate_length.sum())).astype(np.uint8)
    codes[:16] = np.arange(16, dtype=np.uint8)
    return mate_offset, mate_length, codes


def event(query, mate, reversed_, start_a, length, kind=1, contig=0, position=0, weight=1):
    return (contig, position, kind, length, query, mate | (reversed_ << 1), start_a, weight)


def random_events(n, mate_length, seed, query_base=0, deletions=0.3, clipped=0.1, insert_lengths=(1, 1, 2, 3, 5, 63, 64, 65, 1000)):
    """n events over the mates: insertions of the given lengths that fit their mate where it is long enough (else as long as the mate), both mates, both
    orientations; a share of deletions in between; a share of clipped events (startA + length > readLen, startA >= readLen, length 0)."""
    rng = np.random.default_rng(seed)
    nq = len(mate_length) // 2
    out = []
    for k in range(n):
        q, mate, rev = int(rng.integers(0, nq)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        read_len = int(mate_length[2 * q + mate])
        u = rng.random()
        if u < deletions:
            out.append(event(q + query_base, mate, rev, int(rng.integers(0, read_len + 1)), int(rng.integers(1, 9)), kind=2, position=k))
            continue
        length = min(int(insert_lengths[int(rng.integers(0, len(insert_lengths)))]), read_len)
        start = int(rng.choice([0, read_len - length, int(rng.integers(0, read_len - length + 1))]))
        if u < deletions + clipped:
            start, length = [(read_len - length + 1, length), (read_len, 3), (read_len + 7, 2), (start, 0)][int(rng.integers(0, 4))]
        out.append(event(q + query_base, mate, rev, start, length, position=k))
    return np.array(out, np.int64).reshape(-1, 8)


def rule_text(mate_offset, mate_length, codes, events, query_base=0):
    """-> (off[n + 1], text) by the definition; an event of a query outside of the batch, a deletion, and a startA in front of the mate have no text."""
    nq = len(mate_length) // 2
    off, parts = [0], []
    for contig, pos, kind, length, q, flags, start_a, weight in (tuple(int(x) for x in e) for e in events):
        q -= query_base
        text = ""
        if kind == 1 and length > 0 and 0 <= q < nq and start_a >= 0:
            k = 2 * q + (flags & 1)
            mate = codes[mate_offset[k]:mate_offset[k] + mate_length[k]]
            oriented = api.reverse_complement(mate) if (flags >> 1) & 1 else mate
            text = api.decode(oriented[start_a:start_a + length])
        parts.append(text)
        off.append(off[-1] + len(text))
    return np.array(off, np.int64), "".join(parts).encode("ascii")


def event_order(e):
    """The order xm_pileup_add_last documents: (query ordinal, contig, position, flags, startA)."""
    return (e[4], e[0], e[1], e[5], e[6])


def insertion_texts(events, queries_of_ordinal):
    """The text the host derives from the queries for every insertion event (None for a deletion).  queries_of_ordinal(ordinal) -> the mates of that query."""
    out = []
    for e in events:
        if e[2] != 1:
            out.append(None)
            continue
        mate = np.asarray(queries_of_ordinal(e[4])[e[5] & 1], np.uint8)
        oriented = api.reverse_complement(mate) if (e[5] >> 1) & 1 else mate
        out.append(api.decode(oriented[e[6]:e[6] + e[3]]))
    return out


def pairs_with_insertions(seed=0x7E7):
    """1 000 pairs on one contig: 950 from the filler with mates that overlap by 100, 60, 30, 1 and 0 bases or lie 40 apart, fragments from both strands,
    half of them with an indel (two in three an insertion) in mate 1 or mate 2; and 50 from inside families of two and three exact copies, with an insertion
    of two bases in one mate, which align once per copy.  -> (contigs, oracle_lib.QueryBatch)"""
    import oracle_lib
    import pileup_workloads as W
    rng = np.random.default_rng(seed)
    contigs, families = W.family_reference((30_000,), (2, 3), seed)
    ref = contigs[0][1]
    family_at = np.zeros(len(ref), bool)
    for seq, places in families.values():
        for c, at, _ in places:
            family_at[max(at - 450, 0):at + 850] = True
    queries = []
    while len(queries) < 950:
        k = len(queries)
        start = int(rng.integers(0, len(ref) - 350))
        if family_at[start]:
            continue
        kind = (k // len(W.OVERLAP_INNERS)) % 4   # exact, substitutions, an indel in mate 1, an indel in mate 2
        indel = int(rng.choice([2, -1, -2, -3, -4, 3])) if kind >= 2 else 0
        queries.append(W.fragment_pair(ref[start:start + 350], W.OVERLAP_INNERS[k % len(W.OVERLAP_INNERS)], rng, reverse=bool(rng.integers(0, 2)),
                                       subs_in_overlap=2 if kind == 1 else 0, indel=indel, indel_mate=kind - 2 if kind >= 2 else 0))
    for k, (seq, places) in families.items():
        for j in range(25):
            inner = (-100, -60, -30, -1)[j % 4]
            start = int(rng.integers(0, 400 - (300 + inner) - 3))
            queries.append(W.fragment_pair(seq[start:], inner, rng, reverse=bool(j & 8), indel=-2, indel_mate=j & 1))
    order = rng.permutation(len(queries))
    return contigs, oracle_lib.QueryBatch([queries[i] for i in order])


def reads_with_ambiguous_insertions(ref, n, seed):
    """n reads of 150 bases from `ref`, every other one from the other strand, each with N and R inserted in front of a base away from its ends."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        start = int(rng.integers(0, len(ref) - 150))
        at = int(rng.integers(40, 110))
        read = np.concatenate([ref[start:start + at], np.array([15, 5], np.uint8), ref[start + at:start + 148]])
        out.append(api.reverse_complement(read) if k & 1 else read)
    return out
