"""Pairs at the edges of the pairing rules, for tests/test_pair_geometry.py (host simulation against the oracle) and tests/test_gpu_pairs.py (the GPU against
the oracle), and the queries for which the reference would have thrown.

TEST INFRASTRUCTURE ONLY, plain Python.  Everything is a pure function of its seed.  reference() -> (contigs in length-descending order, the places of
the repeat family); every class returns a list of Group: alignment parameters, queries (mates, expected_inner, deviation) and, per query, a tag that
says what the query is there for - the tests assert from the oracle's answer that the tag came true, so that a change here cannot empty a class unnoticed.

The rules the edges are computed from (HashBlockPaths_Counter.java:136-247 as restated in mapper_amd/csrc/xm_seed.h pcMatchWithoutCache; AlignerWorker.java
:602-644 as restated in xm_worker.h getUnpairedAlignments).  With D = (start of mate 2's span) - (start of mate 1's span) on the forward reference, s = +1 for a
fragment from the forward strand and -1 for one from the reverse strand, E = (int)((len1 + len2) * MaxErrorRate * deviation + expected_inner):

    the mates are paired  <=>  -(len of the second component) / 2  <=  s * D  <=  E + len1        (both edges inclusive, integer division)

where the second component is the mate with more candidate positions, mate 2 when both have as many.  A mate whose partner finds nothing is aligned alone
only where  max(distance from its far end to the contig's end, expected_inner) / deviation <= len * MaxErrorRate."""
import collections
import math
import numpy as np

import oracle_lib
from pileup_workloads import CODES, family_reference, fragment_pair, rc   # (fragment_pair puts its substitutions and indels in with substitute and with_indel)

Group = collections.namedtuple("Group", "params queries tags")
SPACING = (100.0, 50.0)
FAMILY = 9
CONTIG_LENGTHS = (50_000, 30_000, 12_000)
NAN, INF = float("nan"), float("inf")


def reference(seed=0x9A12):
    """Three contigs (92 kb) with one family of FAMILY exact copies of a 400-base segment -> (contigs, (segment, [(contig, start, reversed)]))."""
    contigs, families = family_reference(CONTIG_LENGTHS, (FAMILY,), seed)
    return contigs, families[FAMILY]


def j2i(d):
    """(int) of a Java double: truncation, saturation, NaN -> 0"""
    if d != d:
        return 0
    return int(max(-2 ** 31, min(2 ** 31 - 1, math.trunc(d)))) if abs(d) != INF else (2 ** 31 - 1 if d > 0 else -2 ** 31)


def upper_edge(len1, len2, rate, expected, deviation):
    """E: the largest inner distance at which the mates of a forward fragment are still paired."""
    return j2i((len1 + len2) * rate * deviation + expected)


def fallback_cut(length, rate, deviation):
    """The largest distance to the contig's end at which a lone mate of `length` bases is aligned (expected_inner below it): d / deviation <= length * rate."""
    c = int(length * rate * deviation)
    while (c + 1) / deviation <= length * rate:
        c += 1
    while c / deviation > length * rate:
        c -= 1
    return c


class _Layout:
    """Where pairs may be cut from: places away from the family's copies (unique text) and places inside a copy."""

    def __init__(self, seed):
        self.contigs, (self.segment, self.places) = reference()
        self.rng = np.random.default_rng(seed)
        self.family_at = [np.zeros(len(r), bool) for _, r in self.contigs]
        for c, at, _ in self.places:
            self.family_at[c][at:at + len(self.segment)] = True

    def unique_origin(self, before, after, contig=None):
        """(contig, origin) with [origin - before, origin + after) inside the contig, at least 400 bases from its ends and free of family text."""
        for _ in range(10_000):
            c = int(self.rng.integers(0, 2)) if contig is None else contig
            n = len(self.contigs[c][1])
            o = int(self.rng.integers(before + 400, n - after - 400))
            if not self.family_at[c][o - before:o + after].any():
                return c, o
        raise AssertionError("no unique place")

    def family_origin(self, mate, other, lo, hi):
        """(contig, origin) such that the interval `mate` (relative to the origin, as `other`, lo and hi) lies inside a copy of the family - 100 bases into
        it, or, where `other` overlaps it, flush with the copy's end on the side of `other`, which then reaches into unique text -, at least 40 bases of
        `other` are no family text, no other copy lies within hi - lo bases of [lo, hi) (none pairs with the partner) and [lo, hi) keeps 400 bases from the
        contig's ends."""
        for c, at, _ in self.places:
            n = len(self.contigs[c][1])
            if other[1] <= mate[0] or other[0] >= mate[1]:
                o = at + 100 - mate[0]
            else:
                o = at - mate[0] if other[0] < mate[0] else at + len(self.segment) - mate[1]
            if o + lo < 400 or o + hi > n - 400:
                continue
            mask = self.family_at[c].copy()
            mask[at:at + len(self.segment)] = False
            if mask[max(0, o + lo - (hi - lo)):o + hi + (hi - lo)].any() or (~self.family_at[c][o + other[0]:o + other[1]]).sum() < 40:
                continue
            return c, o
        raise AssertionError("no family copy with room for [%d, %d)" % (lo, hi))


def spans(len1, x2, len2, reverse):
    """The reference intervals, relative to the origin, of mate 1 and mate 2 of place_pair."""
    return ((0, len1), (x2, x2 + len2)) if not reverse else ((-len1, 0), (-x2 - len2, -x2))


def place_pair(ref, origin, len1, x2, len2, reverse):
    """Mate 1 covers the fragment's [0, len1) and mate 2 its [x2, x2 + len2), the fragment starting at `origin` and running up the forward strand, or,
    `reverse`, down it (fragment position x is reference position origin - 1 - x, complemented)."""
    if not reverse:
        return [ref[origin:origin + len1].copy(), rc(ref[origin + x2:origin + x2 + len2])]
    return [rc(ref[origin - len1:origin]), ref[origin - x2 - len2:origin - x2].copy()]


def x2_for(t, len1, len2, reverse):
    """The fragment position of mate 2 at which s * D (module docstring) is t."""
    return t + len1 - len2 if reverse else t


# ---------------------------------------------------------------- window_edges

WINDOW_SETTINGS = (  # (len1, len2, MaxErrorRate, expected_inner, deviation)
    (150, 150, 0.1, 100.0, 50.0),     # 300 * 0.1 * 50 + 100 = 1600
    (120, 151, 0.1, 0.0, 10.5),       # 27.1 * 10.5 = 284.55 -> 284
    (151, 121, 0.07, 100.0, 33.3),    # 19.04 * 33.3 + 100 = 734.03 -> 734
    (101, 101, 0.07, 250.0, 7.7),     # 14.14 * 7.7 + 250 = 358.878 -> 358
)


def window_edges(seed=0x3E1):
    """Per setting, strand and candidate shape (both mates unique; mate 1 inside the family, so that mate 1 is the second component; mate 2 inside the
    family): pairs with s * D at E + len1 - 1, E + len1, E + len1 + 1 and at -(h - 1), -h, -(h + 1) with h = (length of the second component) / 2.
    tags: ("upper" | "lower", setting, reverse, shape, -1 | 0 | 1) - the pair at 1 lies outside the window."""
    lay = _Layout(seed)
    groups = {}
    for setting, (len1, len2, rate, exp, dev) in enumerate(WINDOW_SETTINGS):
        e = upper_edge(len1, len2, rate, exp, dev)
        g = groups.setdefault(rate, Group(dict(MaxErrorRate=rate), [], []))
        for reverse in (False, True):
            for shape in ("unique", "family1", "family2"):
                half = (len1 if shape == "family1" else len2) // 2
                for edge, ts in (("upper", (e + len1 - 1, e + len1, e + len1 + 1)), ("lower", (-(half - 1), -half, -(half + 1)))):
                    for side, t in zip((-1, 0, 1), ts):
                        x2 = x2_for(t, len1, len2, reverse)
                        s1, s2 = spans(len1, x2, len2, reverse)
                        lo, hi = min(s1[0], s2[0]) - 5, max(s1[1], s2[1]) + 5
                        if shape == "unique":
                            c, o = lay.unique_origin(-lo, hi)
                        else:
                            c, o = lay.family_origin(s1, s2, lo, hi) if shape == "family1" else lay.family_origin(s2, s1, lo, hi)
                        g.queries.append((place_pair(lay.contigs[c][1], o, len1, x2, len2, reverse), exp, dev))
                        g.tags.append((edge, setting, reverse, shape, side))
    return list(groups.values())


# ---------------------------------------------------------------- spacing_steps

STEP_SETTINGS = ((150, 150, 100.0, 50.0), (131, 150, 250.0, 7.7))   # (len1, len2, expected_inner, deviation)


def spacing_penalty(inner, total_length, expected, deviation):
    """computeSpacingPenalty (QueryMatch_Aligner.java:530-546): nothing for mates that overlap, else (int)(|inner - expected| / deviation)."""
    if -total_length < inner < 0:
        return 0
    return j2i(abs(inner - expected) / deviation)


def spacing_steps(seed=0x3E2):
    """Pairs whose |inner - expected| is k * deviation - 1, k * deviation and k * deviation + 1 (rounded up to whole bases) for k = 1 .. 4, on either
    side of the expected distance, and pairs with inner distance -1, 0 and 1: an overlap costs nothing, a distance of 0 costs its full step.  Both strands.
    tags: ("step", setting, inner, reverse, the penalty computeSpacingPenalty gives)."""
    lay = _Layout(seed)
    g = Group({}, [], [])
    for setting, (len1, len2, exp, dev) in enumerate(STEP_SETTINGS):
        inners = {-1, 0, 1}
        for k in range(1, 5):
            for d in (-1, 0, 1):
                v = math.ceil(k * dev) + d
                inners |= {int(exp) + v, int(exp) - v}
        for inner in sorted(i for i in inners if i > -min(len1, len2) + 20):   # (nothing contained: throwers())
            for reverse in (False, True):
                s1, s2 = spans(len1, len1 + inner, len2, reverse)
                c, o = lay.unique_origin(5 - min(s1[0], s2[0]), max(s1[1], s2[1]) + 5)
                g.queries.append((place_pair(lay.contigs[c][1], o, len1, len1 + inner, len2, reverse), exp, dev))
                g.tags.append(("step", setting, inner, reverse, spacing_penalty(inner, len1 + len2, exp, dev)))
    return [g]


# ---------------------------------------------------------------- joins

def mates_agree(mates, overlap):
    """Do the last `overlap` bases of mate 1 equal the first `overlap` bases of mate 2's reverse complement (tryJoinQuerySequences joins such mates)?  An FR
    pair reads the same from either strand: this holds for fragments of both."""
    a, b = mates[0], rc(mates[1])
    return 0 < overlap <= min(len(a), len(b)) and bool(np.array_equal(a[len(a) - overlap:], b[:overlap]))


def contained_pair(ref, origin, a, container_is_mate_1, reverse, inner_length=80):
    """One mate covers the reference's [origin, origin + 150), the other [origin + a, origin + a + inner_length) inside it, on the other strand."""
    outer, inner = ref[origin:origin + 150].copy(), ref[origin + a:origin + a + inner_length].copy()
    if container_is_mate_1:
        return [rc(outer), inner] if reverse else [outer, rc(inner)]
    return [rc(inner), outer] if reverse else [inner, rc(outer)]


def contained_throws(a, container_is_mate_1, reverse, inner_length=80):
    """The rule for contained_pair, from pcMatchWithoutCache's window and tryJoinQuerySequences: the mates are paired when mate 2 starts no more than half
    its length on the wrong side of mate 1's start, and the join then asks for a range of negative length when the contained mate ends before its partner
    does and either starts behind its partner's start or is mate 2."""
    d = a if container_is_mate_1 else -a                      # start of mate 2 - start of mate 1
    len2 = inner_length if container_is_mate_1 else 150
    in_window = (-d if reverse else d) >= -(len2 // 2)
    return in_window and a + inner_length < 150 and (a > 0 or container_is_mate_1)


def joins(seed=0x3E3):
    """Mates that overlap (tryJoinQuerySequences, QueryMatch_Aligner.java:274-319): by 1, 2, length - 1 bases and wholly (offset 0: mate 2 is the reverse
    complement of mate 1); mate 2 shorter without being contained; a substitution inside the overlap (the mates are not joinable and are aligned one by
    one); an indel inside the overlap; each from either strand - from the reverse strand the offset between the mates is negative and they swap roles.
    And a mate contained in its partner where the reference does not throw for it (contained_throws): flush with its partner's end, and the like.
    tags: ("join", overlap, kind, reverse, do the mates agree over the overlap)."""
    lay = _Layout(seed)
    rng = lay.rng
    g = Group({}, [], [])
    for rep in range(3):
        for reverse in (False, True):
            for overlap, kind, kw in ((1, "exact", {}), (2, "exact", {}), (149, "exact", {}), (150, "exact", {}), (60, "exact", {}),
                                      (100, "shorter", dict(trim=25)), (30, "shorter", dict(trim=25)), (149, "shorter", dict(trim=1)),
                                      (60, "substitution", dict(subs_in_overlap=1)), (100, "substitution", dict(subs_in_overlap=2)), (2, "substitution", dict(subs_in_overlap=1)),
                                      (100, "indel1", dict(indel=2, indel_mate=0)), (100, "indel2", dict(indel=-2, indel_mate=1)), (60, "indel2", dict(indel=3, indel_mate=1))):
                c, o = lay.unique_origin(5, 360)
                mates, exp, dev = fragment_pair(lay.contigs[c][1][o:o + 350], -overlap, rng, reverse, **kw)
                overlap -= kw.get("trim", 0)
                g.queries.append((mates, exp, dev))
                g.tags.append(("join", overlap, kind, reverse, mates_agree(mates, overlap)))
    for reverse in (False, True):
        for container_is_mate_1 in (True, False):
            for a in (0, 20, 70):
                if not contained_throws(a, container_is_mate_1, reverse):
                    c, o = lay.unique_origin(5, 160, contig=1)
                    g.queries.append((contained_pair(lay.contigs[c][1], o, a, container_is_mate_1, reverse), SPACING[0], SPACING[1]))
                    g.tags.append(("contained", a, "mate 2 in mate 1" if container_is_mate_1 else "mate 1 in mate 2", reverse, True))
    return [g]


# ---------------------------------------------------------------- orientation_and_contigs

def orientation_and_contigs(seed=0x3E4):
    """Pairs the rules do not pair, and pairs at the contigs' ends: both mates on the same strand (FF, RR), facing outwards (RF), on different contigs;
    a mate that hangs 1, 20 and 50 bases over either end of a contig (junk beyond it) with its partner inside; identical mates, and a mate with its own
    reverse complement; a pair with a mate at either end of the contig, which fall back
    to two unpaired alignments.  FR pairs beside them.  tags: (kind, detail)."""
    lay = _Layout(seed)
    rng = lay.rng
    g = Group({}, [], [])

    def add(mates, tag):
        g.queries.append((mates, SPACING[0], SPACING[1]))
        g.tags.append(tag)

    for rep in range(4):
        c, o = lay.unique_origin(5, 460)
        ref = lay.contigs[c][1]
        a, b = ref[o:o + 150].copy(), ref[o + 250:o + 400].copy()   # (forward texts of an FR pair 100 apart)
        add([a, rc(b)], ("FR", rep))
        add([rc(b), a], ("FR", rep + 4))
        add([a, b], ("FF", rep))
        add([rc(a), rc(b)], ("RR", rep))
        add([rc(a), b], ("RF", rep))
        add([b, rc(a)], ("RF", rep + 4))
        add([a.copy(), a.copy()], ("identical", rep))
        add([a, rc(a)], ("own reverse complement", rep))
        c2, o2 = lay.unique_origin(5, 160, contig=2)
        add([a, rc(lay.contigs[c2][1][o2:o2 + 150])], ("two contigs", rep))
    for c, (_, ref) in enumerate(lay.contigs):
        n = len(ref)
        for over in (1, 20, 50):
            junk = CODES[rng.integers(0, 4, over)]
            add([np.concatenate([junk, ref[:150 - over]]), rc(ref[250:400])], ("over the start", c, over, "mate 1"))
            add([rc(ref[250:400]), np.concatenate([junk, ref[:150 - over]])], ("over the start", c, over, "mate 2"))   # (a reverse-strand fragment)
            add([rc(ref[n - 400:n - 250]), rc(np.concatenate([junk, ref[:150 - over]]))], ("both ends", c, over))       # (each mate falls back on its own)
            add([ref[n - 400:n - 250].copy(), rc(np.concatenate([ref[n - 150 + over:], junk]))], ("over the end", c, over, "mate 2"))
            add([rc(np.concatenate([ref[n - 150 + over:], junk])), ref[n - 400:n - 250].copy()], ("over the end", c, over, "mate 1"))
    return [g]


# ---------------------------------------------------------------- fallback_edges

FALLBACK_SETTINGS = ((100.0, 50.0), (20.0, 7.7))   # (expected_inner, deviation)
FALLBACK_LENGTHS = (150, 101)


def fallback_edges(seed=0x3E5):
    """The two shapes of pileup_workloads.fallback_pairs - mate 1 forward before the contig's end with a junk mate 2 (1, 0); mate 2 the reverse complement
    of a piece behind the contig's start with a junk mate 1 (0, 1) - at distances c - 1, c and c + 1 from the contig's end, c = fallback_cut();
    and at 10 bases from the end with an expected inner distance at, and one past, the cut.  tags: ("fallback", shape, contig, length, -1 | 0 | 1): the
    mate at 1 is not aligned."""
    lay = _Layout(seed)
    rng = lay.rng
    g = Group({}, [], [])
    rate = 0.1
    for c, (_, ref) in enumerate(lay.contigs):
        n = len(ref)
        for exp, dev in FALLBACK_SETTINGS:
            for length in FALLBACK_LENGTHS:
                cut = fallback_cut(length, rate, dev)
                places = [(cut + side, exp, side) for side in (-1, 0, 1)]
                places += [(10, float(cut), 0), (10, float(cut + 1), 1)]
                for dist, e, side in places:
                    g.queries.append(([ref[n - dist - length:n - dist].copy(), CODES[rng.integers(0, 4, length)]], e, dev))
                    g.tags.append(("fallback", (1, 0), c, length, side))
                    g.queries.append(([CODES[rng.integers(0, 4, length)], rc(ref[dist:dist + length])], e, dev))
                    g.tags.append(("fallback", (0, 1), c, length, side))
    return [g]


# ---------------------------------------------------------------- odd_spacing and the throwers

ODD_DEVIATIONS = (0.0, 1e-9, 1e-3, 4.3e7, NAN)
ODD_EXPECTED = (-1000.0, -1.0, 1e12, -1e12, NAN, INF, -INF)


def _ordinary_pairs(lay, count):
    """FR pairs of 150-base mates 0 .. 300 apart from unique text, alternately from either strand -> [(mates, reverse)]."""
    out = []
    for k in range(count):
        inner = int(lay.rng.integers(0, 301))
        c, o = lay.unique_origin(460, 460)
        out.append((place_pair(lay.contigs[c][1], o, 150, 150 + inner, 150, bool(k & 1)), bool(k & 1)))
    return out


def spacing_throws(expected, deviation, reverse):
    """Does the window of pcMatchWithoutCache wrap for a pair of 150-base mates (searchStart > searchEnd: TreeMap.subMap throws)?  In Java's 32-bit
    arithmetic, for offsets small against 2^31: a negative reach on either strand, and a reach of 2^31 or more on a reversed fragment."""
    wrap = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31
    reach = wrap(j2i(300 * 0.1 * deviation + expected) + 150)
    offset = 20_000
    if reverse:
        return offset - 75 > wrap(offset + reach)
    return wrap(offset - reach) > offset + 75


def odd_spacing(seed=0x3E6):
    """Ordinary pairs from both strands, every third with the ordinary spacing, the others with one value of ODD_DEVIATIONS for the deviation or one of
    ODD_EXPECTED for the expected inner distance.  Where a value makes the window wrap, whether the reference throws depends on which mate has more
    candidates at the moment: split_throwers() asks the oracle, query by query, and the throwers join throwers().  tags: ("odd", expected_inner, deviation, reverse)."""
    lay = _Layout(seed)
    settings = [(SPACING[0], d) for d in ODD_DEVIATIONS] + [(e, SPACING[1]) for e in ODD_EXPECTED]
    g = Group({}, [], [])
    for rep in range(4):
        for exp, dev in settings:
            for mates, reverse in _ordinary_pairs(lay, 2):
                g.queries.append((mates, exp, dev))
                g.tags.append(("odd", exp, dev, reverse))
            mates, reverse = _ordinary_pairs(lay, 1)[0]
            g.queries.append((mates, SPACING[0], SPACING[1]))
            g.tags.append(("odd", SPACING[0], SPACING[1], reverse))
    return [g]


def split_throwers(oracle, group):
    """-> (the Group without the queries for which `oracle` (an oracle_lib.OracleReference) throws when it aligns them alone, [(tag, query, text)] of those)."""
    params = oracle_lib.make_params(group.params)
    keep, thrown = Group(group.params, [], []), []
    for q, tag in zip(group.queries, group.tags):
        try:
            oracle.align(oracle_lib.QueryBatch([q]), params)
            keep.queries.append(q)
            keep.tags.append(tag)
        except RuntimeError as e:
            thrown.append((tag, q, str(e)))
    return keep, thrown


NEGATIVE_LENGTH = "getRange with negative length"
WRAPPED_WINDOW = "subMap: fromKey > toKey"


def throwers(seed=0x3E7):
    """Single queries for which the reference throws -> [(kind, query, text of the oracle's exception)].  A mate that lies inside its partner where
    tryJoinQuerySequences asks for a range of negative length (contained_throws): mate 2 inside mate 1 and mate 1 inside mate 2, fragments from both strands,
    in the middle of the partner and flush with its start; a negative deviation on either strand; a deviation, or an expected inner distance, so large that
    the window's 32-bit arithmetic wraps (spacing_throws: fragments from the reverse strand)."""
    lay = _Layout(seed)
    out = []
    for reverse in (False, True):
        for container_is_mate_1 in (True, False):
            for a in (0, 20, 70):
                if contained_throws(a, container_is_mate_1, reverse):
                    c, o = lay.unique_origin(5, 160)
                    kind = "contained: %s, %d bases in, %s strand" % ("mate 2 in mate 1" if container_is_mate_1 else "mate 1 in mate 2", a, "reverse" if reverse else "forward")
                    out.append((kind, (contained_pair(lay.contigs[c][1], o, a, container_is_mate_1, reverse), SPACING[0], SPACING[1]), NEGATIVE_LENGTH))
    for (mates, reverse), dev in zip(_ordinary_pairs(lay, 4), (-50.0, -50.0, -1000.0, -INF)):
        assert spacing_throws(SPACING[0], dev, reverse)
        out.append(("negative deviation %r, %s strand" % (dev, "reverse" if reverse else "forward"), (mates, SPACING[0], dev), WRAPPED_WINDOW))
    for exp, dev in [(SPACING[0], d) for d in (7.2e7, 1e12, INF)] + [(e, SPACING[1]) for e in (1e12, -1e12)]:
        mates, reverse = _ordinary_pairs(lay, 2)[1]
        assert reverse and spacing_throws(exp, dev, reverse)
        out.append(("wrapped window: expected %r, deviation %r, reverse strand" % (exp, dev), (mates, exp, dev), WRAPPED_WINDOW))
    return out


THROWER_KINDS = ("contained", "negative deviation", "wrapped window")


def ordinary_queries(count, seed=0x3E8):
    """`count` queries the reference aligns: FR pairs 0 .. 300 apart from either strand with the ordinary spacing, every fifth query a single read."""
    lay = _Layout(seed)
    out = []
    for k, (mates, _) in enumerate(_ordinary_pairs(lay, count)):
        out.append(([mates[k & 1]], 0.0, 1.0) if k % 5 == 4 else (mates, SPACING[0], SPACING[1]))
    return out


def with_throwers(ordinary, placed):
    """The queries `ordinary` with, for every (index, query) of `placed`, the query put in at that index of the result -> list of queries."""
    out = list(ordinary)
    for at, q in sorted(placed, key=lambda x: x[0]):
        out.insert(at, q)
    return out


def one_of_each_kind(thrown=None):
    """-> {kind of THROWER_KINDS: (query, text)}: the first thrower of each kind."""
    out = {}
    for kind, q, text in throwers() if thrown is None else thrown:
        out.setdefault(next(k for k in THROWER_KINDS if kind.startswith(k)), (q, text))
    return out


CLASSES = dict(window_edges=window_edges, spacing_steps=spacing_steps, joins=joins, orientation_and_contigs=orientation_and_contigs, fallback_edges=fallback_edges,
               odd_spacing=odd_spacing)


def batch(group):
    return oracle_lib.QueryBatch(group.queries)
