"""Inputs of the pile-up comparison (tests/test_gpu_pileup.py: device counts against tests/pileup_model.py) and the conditions each of them exists for.

TEST INFRASTRUCTURE ONLY.  Every workload is a pure function of its seeds: contigs [(name, codes)] in length-descending order and one or more
oracle_lib.QueryBatch.  The condition checkers take decoded alignments and counts, whoever made them (the GPU in the GPU tier, the oracle when an
input is tried on the CPU), and return what they found so that a test can assert on it."""
import numpy as np

import helpers
import oracle_lib
from mapper_amd import api, synth
from pileup_model import UNIT

CODES = np.array([1, 2, 4, 8], np.uint8)
PAIR_SPACING = (100.0, 50.0)   # expected inner distance and deviation per unit of penalty (what the fallback shapes were tried with)
FAMILY_SIZES = (2, 3, 5, 7, 11, 13, 16, 17, 19, 23)
OVERLAP_INNERS = (-100, -60, -30, -1, 0, 40)


def rc(codes):
    return api.reverse_complement(codes)


def substitute(read, positions, rng):
    """`read` with another unambiguous base at each of `positions`."""
    out = read.copy()
    for p in positions:
        others = CODES[CODES != out[p]] if out[p] in (1, 2, 4, 8) else CODES
        out[p] = others[rng.integers(0, len(others))]
    return out


def with_indel(template, length, at, n, rng):
    """`length` bases from `template` (at least length + n long) with, in front of index `at`, n bases deleted (n > 0) or -n random bases inserted."""
    if n > 0:
        t = np.concatenate([template[:at], template[at + n:]])
    elif n < 0:
        t = np.concatenate([template[:at], CODES[rng.integers(0, 4, -n)], template[at:]])
    else:
        t = template
    return t[:length].copy()


def mates_of(batch):
    """The mates of every query of a QueryBatch, as code arrays."""
    return [[batch.codes[batch.mate_offset[2 * q + m]:batch.mate_offset[2 * q + m] + batch.mate_length[2 * q + m]] for m in range(int(batch.mate_count[q]))]
            for q in range(batch.nq)]


def single(read):
    return ([read], 0.0, 1.0)


def pair(m1, m2):
    return ([m1, m2], PAIR_SPACING[0], PAIR_SPACING[1])


def noisy_reads(ref, n, seed, indel_prob=0.3):
    """n single reads of 150 bases from anywhere in `ref`, either strand, 1 % substitutions and an indel in `indel_prob` of them (synth.synthetic_single_end:
    the generator whose indels reach into the end zones of the reads)."""
    return [single(r) for r in synth.synthetic_single_end(ref, n, seed=seed, indel_prob=indel_prob)[0]]


def edited_read(ref, start, rng, reverse, subs=1, indel=0, length=150):
    """A read of `length` bases from ref[start:], with `subs` substitutions and an indel of `indel` bases (deleted > 0, inserted < 0) away from its ends."""
    read = with_indel(ref[start:start + length + max(indel, 0)], length, int(rng.integers(30, length - 30)), indel, rng)
    read = substitute(read, rng.integers(20, length - 20, subs), rng)
    return rc(read) if reverse else read


# ---------------------------------------------------------------- a. several contigs

def several_contigs(seed=0xA11):
    """Three contigs of different lengths; reads with substitutions and indels on both strands; per contig, reads cut at [0, 150) and [len - 150, len) on
    both strands, exact and with a substitution.  No read starts in [150, 400) or ends in [len - 400, len - 150): the pile-up has positions that no read
    reaches next to the covered ends of every contig."""
    rng = np.random.default_rng(seed)
    contigs = [("c%d" % i, synth.synthetic_reference(n, seed=seed + i)) for i, n in enumerate((12_000, 7_000, 3_100))]
    queries = []
    for c, (_, ref) in enumerate(contigs):
        n = len(ref)
        for k in range(int(n / 5)):  # (depth about 30)
            start = int(rng.integers(400, n - 400 - 153))
            queries.append(single(edited_read(ref, start, rng, reverse=bool(k & 1), subs=int(rng.integers(0, 3)), indel=int(rng.choice([0, 0, 0, 1, 2, 3, -1, -2, -3])))))
        inner = ref[400:n - 400]
        queries += noisy_reads(inner, int(n / 25), seed + 16 + c)
        for reverse in (False, True):
            for subs in (0, 1):
                queries.append(single(edited_read(ref, 0, rng, reverse, subs)))
                queries.append(single(edited_read(ref, n - 150, rng, reverse, subs)))
    order = rng.permutation(len(queries))
    return contigs, [oracle_lib.QueryBatch([queries[i] for i in order])]


def unreached(contigs):
    """Per contig, the positions that no read of several_contigs() can reach."""
    out = []
    for _, ref in contigs:
        m = np.zeros(len(ref), bool)
        m[150:400] = True
        m[len(ref) - 400:len(ref) - 150] = True
        out.append(m)
    return out


# ---------------------------------------------------------------- b. pairs with overlapping mates

def family_reference(lengths, sizes, seed, segment=400, slot=1000):
    """Contigs of i.i.d. filler with, for every k of `sizes`, a family of k exact copies of a `segment`-base sequence: alternately forward and
    reverse-complemented, one copy per slot of `slot` bases, the slots dealt over all contigs.  -> (contigs, families): families[k] = (sequence,
    [(contig, start, reversed)])."""
    rng = np.random.default_rng(seed)
    refs = [synth.synthetic_reference(n, seed=seed + 1 + i).copy() for i, n in enumerate(lengths)]
    slots = [(c, s * slot + (slot - segment) // 2) for c, n in enumerate(lengths) for s in range(n // slot)]
    assert sum(sizes) <= len(slots)
    order = rng.permutation(len(slots))
    families, used = {}, 0
    for k in sizes:
        seq = CODES[rng.integers(0, 4, segment)]
        places = []
        for j in range(k):
            c, at = slots[order[used]]
            used += 1
            refs[c][at:at + segment] = rc(seq) if j & 1 else seq
            places.append((c, at, bool(j & 1)))
        families[k] = (seq, places)
    return [("c%d" % i, r) for i, r in enumerate(refs)], families


def fragment_pair(region, inner, rng, reverse, subs_in_overlap=0, indel=0, indel_mate=0, length=150, trim=0):
    """An FR pair from `region` (forward reference bases, at least 2 * length + inner + 3): mate 1 = region[0 : length], mate 2 = the reverse complement
    of region[length + inner : 2 * length + inner]; `reverse`: the fragment comes from the other strand (the mates swap roles).  Substitutions and the
    indel go inside the overlap [length + inner, length) when there is one.  `trim`: mate 2 loses that many bases at its 3' end (mates of different lengths)."""
    lo, hi = length + inner, length
    first = region[:length + 3]
    second = region[lo:lo + length + 3]
    at1 = int(rng.integers(lo + 3, hi - 3)) if hi - lo > 12 else int(rng.integers(30, length - 30))
    a = with_indel(first, length, at1, indel if indel_mate == 0 else 0, rng)
    at2 = at1 - lo if hi - lo > 12 else int(rng.integers(30, length - 30))
    b = with_indel(second, length, at2, indel if indel_mate == 1 else 0, rng)
    if subs_in_overlap and hi - lo > 0:
        for _ in range(subs_in_overlap):
            p = int(rng.integers(lo, hi))   # a reference offset inside the overlap, substituted in one of the mates
            if rng.integers(0, 2) and not (indel and indel_mate == 0):
                a = substitute(a, [p], rng)
            elif not (indel and indel_mate == 1):
                b = substitute(b, [p - lo], rng)
    b = b[trim:]
    return pair(rc(b), a) if reverse else pair(a, rc(b))


def overlapping_pairs(seed=0xB22):
    """Pairs whose mates overlap by 100, 60, 30, 1 and 0 bases (and pairs 40 apart), fragments from both strands, substitutions and indels inside the
    overlap, half of the pairs with a mate 2 that is 25 or 60 bases shorter than mate 1, on two contigs; and the same pairs from inside families of 17 and 19 copies, whose alignments carry odd weights (1441440 // 19 = 75865;
    1441440 // 17 + 1 = 84791 for the first ten of 17), so that w // 2 and w - w // 2 differ."""
    rng = np.random.default_rng(seed)
    contigs, families = family_reference((80_000, 40_000), (17, 19), seed)
    family_at = [np.zeros(len(r), bool) for _, r in contigs]
    for seq, places in families.values():
        for c, at, _ in places:
            family_at[c][at - 450:at + 850] = True
    queries = []
    for c, (_, ref) in enumerate(contigs):
        for k in range(len(ref) // 25):
            inner = OVERLAP_INNERS[k % len(OVERLAP_INNERS)]
            start = int(rng.integers(0, len(ref) - 350))
            if family_at[c][start]:
                continue
            kind = (k // len(OVERLAP_INNERS)) % 4   # exact, substitutions, an indel in mate 1, an indel in mate 2
            indel = int(rng.choice([1, 2, 3, -1, -2, -3])) if kind >= 2 else 0
            queries.append(fragment_pair(ref[start:start + 350], inner, rng, reverse=bool(rng.integers(0, 2)), subs_in_overlap=2 if kind == 1 else 0, indel=indel, indel_mate=kind - 2 if kind >= 2 else 0, trim=(0, 0, 25, 60)[(k // 24) % 4]))
        queries += noisy_reads(ref, len(ref) // 200, seed + 32 + c)
    for k, (seq, places) in families.items():
        for j in range(48):
            inner = (-100, -60, -30, -1)[j % 4]
            start = int(rng.integers(0, 400 - (300 + inner) - 3))
            kind = (j // 4) % 3
            indel = int(rng.choice([2, 3, -2])) if kind == 2 else 0
            queries.append(fragment_pair(seq[start:], inner, rng, reverse=bool(j & 8), subs_in_overlap=1 if kind == 1 else 0, indel=indel, indel_mate=j & 1))
    order = rng.permutation(len(queries))
    return contigs, [oracle_lib.QueryBatch([queries[i] for i in order])]


# ---------------------------------------------------------------- c. queries with many equal alignments

def many_equal_alignments(seed=0xC33):
    """Three contigs with a family of k exact copies of a 400-base segment for every k of FAMILY_SIZES (copies alternately forward and reverse-complemented);
    150-base reads from inside each segment - exact, with one substitution, with a 3-base deletion -, pairs from inside each family, and reads from the filler."""
    rng = np.random.default_rng(seed)
    contigs, families = family_reference((70_000, 45_000, 25_000), FAMILY_SIZES, seed)
    queries = []
    for k, (seq, places) in families.items():
        for j in range(120):
            start = int(rng.integers(0, 400 - 153))
            variant = j % 3
            read = with_indel(seq[start:start + 153], 150, int(rng.integers(40, 110)), 3 if variant == 2 else 0, rng)
            if variant == 1:
                read = substitute(read, [int(rng.integers(20, 130))], rng)
            queries.append(single(rc(read) if j & 4 else read))
        for j in range(24):
            inner = (-100, -60, -30, 40)[j % 4]
            start = int(rng.integers(0, 400 - (300 + inner) - 3))
            queries.append(fragment_pair(seq[start:], inner, rng, reverse=bool(j & 4), subs_in_overlap=j % 3, indel=3 if j % 6 == 5 else 0, indel_mate=(j // 6) & 1))
    for c, (_, ref) in enumerate(contigs):
        queries += noisy_reads(ref, len(ref) // 150, seed + 48 + c)
    order = rng.permutation(len(queries))
    return contigs, [oracle_lib.QueryBatch([queries[i] for i in order])]


# ---------------------------------------------------------------- d. pairs that fall back to unpaired alignments

FALLBACK_DISTANCES = tuple(range(0, 701, 50))


def fallback_pairs(seed=0xD44):
    """The reference aligns a lone mate only where its partner could hang off the contig.  On each of three contigs, for every distance of
    FALLBACK_DISTANCES: mate 1 forward ending that many bases before the contig's end with a junk mate 2 (components (1, 0)), and mate 2 given as the
    reverse complement of a piece starting that many bases after the contig's start with a junk mate 1 (components (0, 1)); the aligning mate carries
    substitutions and, in half of the pairs, an indel.  Ordinary pairs fill the rest."""
    rng = np.random.default_rng(seed)
    contigs = [("c%d" % i, synth.synthetic_reference(n, seed=seed + i)) for i, n in enumerate((9_000, 6_000, 4_000))]
    queries = []
    for c, (_, ref) in enumerate(contigs):
        n = len(ref)
        for dist in FALLBACK_DISTANCES:
            for rep in range(8):
                junk = CODES[rng.integers(0, 4, 150)]
                indel = (0, 2, -2, 0, 3, 0, -1, 0)[rep]
                subs = rng.integers(25, 125, 2)
                # (1, 0): the template ends at n - dist; a deletion takes its extra bases from the front
                t = ref[n - dist - 150 - max(indel, 0):n - dist]
                read = with_indel(t, 150 + max(-indel, 0), int(rng.integers(40, 110)), indel, rng)[-150:]
                queries.append(pair(substitute(read, subs, rng), junk))
                # (0, 1): the template starts at dist
                t = ref[dist:dist + 150 + max(indel, 0)]
                read = with_indel(t, 150, int(rng.integers(40, 110)), indel, rng)
                queries.append(pair(CODES[rng.integers(0, 4, 150)], rc(substitute(read, subs, rng))))
        m1, m2 = synth.synthetic_paired_end(ref, n // 20, seed=seed + 64 + c, indel_prob=0.3)[:2]
        queries += [pair(a, b) for a, b in zip(m1, m2)]
    order = rng.permutation(len(queries))
    return contigs, [oracle_lib.QueryBatch([queries[i] for i in order])]


# ---------------------------------------------------------------- e. ambiguity codes

def ambiguous_reads_and_reference(seed=0xE55):
    """Two contigs with N-runs and IUPAC codes (helpers.ambiguous_reference), reads with ambiguity codes sprinkled in (helpers.sprinkle_ambiguity)."""
    contigs = [("c0", helpers.ambiguous_reference(26_000, seed, n_runs=10, n_codes=260)), ("c1", helpers.ambiguous_reference(11_000, seed + 1, n_runs=5, n_codes=110))]
    queries = []
    for c, (_, ref) in enumerate(contigs):
        reads = synth.synthetic_single_end(ref, len(ref) // 8, seed=seed + 8 + c, indel_prob=0.3)[0]
        queries += [single(r) for r in helpers.sprinkle_ambiguity(reads, seed=seed + 16 + c)]
    order = np.random.default_rng(seed).permutation(len(queries))
    return contigs, [oracle_lib.QueryBatch([queries[i] for i in order])]


# ---------------------------------------------------------------- f. long reads

def long_reads(seed=0xF66):
    """300 sections of 1 kb from thirty 10 kb reads with substitutions and indels at rates that align (helpers.long_read_batch), two contigs."""
    contigs = [("c0", synth.synthetic_reference(90_000, seed=seed)), ("c1", synth.synthetic_reference(40_000, seed=seed + 1))]
    a = helpers.long_read_batch(contigs[0][1], 20, 0.01, 0.004, seed=seed + 2)
    b = helpers.long_read_batch(contigs[1][1], 10, 0.01, 0.004, seed=seed + 3)
    return contigs, [oracle_lib.QueryBatch([single(m[0]) for m in mates_of(a) + mates_of(b)])]


# ---------------------------------------------------------------- g. several batches into one pile-up

def three_batches(seed=0x677):
    """Three batches for one pile-up: 700 reads with indels over three contigs, 40 reads of which none aligns, and one read with a deletion."""
    rng = np.random.default_rng(seed)
    contigs = [("c%d" % i, synth.synthetic_reference(n, seed=seed + i)) for i, n in enumerate((8_000, 5_000, 2_500))]
    first = []
    for c, (_, ref) in enumerate(contigs):
        first += noisy_reads(ref, (400, 200, 100)[c], seed + 8 + c, indel_prob=0.5)
    junk = [single(CODES[rng.integers(0, 4, 150)]) for _ in range(40)]
    last = [single(edited_read(contigs[2][1], 1000, rng, reverse=True, subs=1, indel=3))]
    return contigs, [oracle_lib.QueryBatch([first[i] for i in rng.permutation(len(first))]), oracle_lib.QueryBatch(junk), oracle_lib.QueryBatch(last)]


# ---------------------------------------------------------------- the conditions

def sequence_alignments(alignments):
    """(query, component, components of the query, alignments of the component, alignment index, sequence index, QueryAlignment, SequenceAlignment)."""
    for q, comps in enumerate(alignments):
        for c, als in enumerate(comps):
            for a, al in enumerate(als):
                for k, sa in enumerate(al.components):
                    yield q, c, len(comps), len(als), a, k, al, sa


def alignment_counts(alignments):
    """The numbers of alignments that occur in a component."""
    return set(len(als) for comps in alignments for als in comps if als)


def overlaps(alignments):
    """-> (overlap lengths that occur between the two sequences of a pair alignment, number of indel blocks whose startB lies inside such an overlap,
    number of overlaps that split an odd weight)."""
    lengths, indels, odd = set(), 0, 0
    for comps in alignments:
        for als in comps:
            for a, al in enumerate(als):
                s = al.components
                if len(s) != 2 or s[0].contig != s[1].contig:
                    continue
                lo, hi = max(x.start_index_b() for x in s), min(x.end_index_b() for x in s)
                if lo >= hi:
                    continue
                lengths.add(hi - lo)
                w = UNIT // len(als) + (1 if a < UNIT % len(als) else 0)
                odd += w & 1
                indels += sum(1 for x in s for b in x.sections if b.lengthA != b.lengthB and lo <= b.startB < hi)
    return lengths, indels, odd


def fallback_shapes(alignments, mates, contigs):
    """-> set of (contig, shape) with shape (1, 0) or (0, 1): queries of two components of which one is empty, whose aligned mate shows at least one
    substitution against the contig under an equal-length block."""
    found = set()
    for q, comps in enumerate(alignments):
        if len(comps) != 2 or bool(comps[0]) == bool(comps[1]):
            continue
        c = 0 if comps[0] else 1
        for al in comps[c]:
            for sa in al.components:
                read = rc(mates[q][c]) if sa.reference_reversed else mates[q][c]
                ref = contigs[sa.contig][1]
                if any(np.any(read[b.startA:b.startA + b.lengthA] != ref[b.startB:b.startB + b.lengthB]) for b in sa.sections if b.lengthA == b.lengthB):
                    found.add((sa.contig, (1, 0) if c == 0 else (0, 1)))
    return found


def ambiguous_positions(alignments, mates, contigs):
    """-> (aligned positions with an ambiguous read base, aligned positions with an ambiguous reference base), counted per alignment."""
    unambiguous = np.zeros(16, bool)
    unambiguous[[1, 2, 4, 8]] = True
    in_read = in_ref = 0
    for q, c, ncomp, nal, a, k, al, sa in sequence_alignments(alignments):
        m = mates[q][c if ncomp > 1 else k]
        read = rc(m) if sa.reference_reversed else m
        ref = contigs[sa.contig][1]
        for b in sa.sections:
            if b.lengthA == b.lengthB:
                in_read += int((~unambiguous[read[b.startA:b.startA + b.lengthA]]).sum())
                in_ref += int((~unambiguous[ref[b.startB:b.startB + b.lengthB]]).sum())
    return in_read, in_ref


def end_zone_shapes(events, depth, middle):
    """-> (events with flag bit 2, events without, positions where the middle depth is neither 0 nor the depth)."""
    flagged = sum(1 for e in events if e[5] & 4)
    partial = sum(int(((m != 0) & (m != d)).sum()) for d, m in zip(depth, middle))
    return flagged, len(events) - flagged, partial
