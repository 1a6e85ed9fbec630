"""The host half of the pile-up without a GPU: oracle alignments -> tests/pileup_model.py (a plain recount from the documented rules) ->
pileup.CountedMatchDatabase (event grouping, thresholds, continuation cut, line order).  The fixture cases tie the model to what the reference's own
tests pin (tests/golden/mutations_reference.json); the hand-written cases pin the rules the fixtures do not reach, with the expected arrays written out."""
import io
import json
import os
import numpy as np
import pytest

import oracle_lib
import pileup_model
from pileup_model import UNIT, PileupModel
from mapper_amd import api, pileup

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "mutations_reference.json")))

A, C_, G, T, N = 1, 2, 4, 8, 15


def seq_al(contig, reversed_, blocks):
    return api.SequenceAlignment(contig, reversed_, [api.AlignedBlock(*b) for b in blocks], 0.0, 0.0)


def q_al(*seqs):
    return api.QueryAlignment(list(seqs), 0.0, 1.0, 0.0, 0.0, 0)


def counted(model, batches=()):
    return pileup.CountedMatchDatabase(model.contigs, model.depth, model.alt, model.middle, model.sorted_events(), batches, model.f)


def lines_of(m, parameters=None):
    out = io.StringIO()
    m.write_mutations(out, parameters)
    return [l for l in out.getvalue().split("\n") if l and not l.startswith("#") and not l.startswith("CHR")]  # (withoutMetadataLines, MutationsWriter_Test.java:144-154)


def oracle_model(queries, reference, params, fraction=0.0):
    """queries: [(mates, expected inner, deviation)] aligned by the oracle on one contig `ref` (Api.newDatabase's assembly) and recounted."""
    contigs = [("ref", api.encode(reference))]
    batch = oracle_lib.QueryBatch(queries)
    st = oracle_lib.OracleReference(contigs, mode="api").align(batch, oracle_lib.make_params(params))
    alignments = [api.decode_streams(st.ints, st.dbls, st.int_off, st.dbl_off, q) for q in range(batch.nq)]
    mates = [[api.encode(m) if isinstance(m, str) else m for m in q[0]] for q in queries]
    model = PileupModel(contigs, fraction)
    model.add(alignments, mates)
    return model, alignments, mates


# ---------------------------------------------------------------- the reference's fixtures through oracle -> model -> host writer

@pytest.mark.parametrize("case", FIX["mutation_cases"], ids=[c["name"] for c in FIX["mutation_cases"]])
def test_fixture_mutation_cases_through_oracle_and_model(case):
    f = case.get("query_end_fraction", 0.0)
    model, alignments, mates = oracle_model([([case["query"]], 0.0, 1.0)], case["reference"], FIX["alignment_parameters"], f)
    assert len(alignments[0]) == 1 and len(alignments[0][0]) >= 1  # (testOneMutation's query is its own reverse complement: two alignments of 1/2 each)
    m = counted(model, [[api.Query(*mates[0])]])
    assert lines_of(m, pileup.MutationDetectionParameters(**case.get("filter", {}))) == case["expected"]


def test_fixture_match_database_cases_through_oracle_and_model():
    c = FIX["match_database_cases"][0]
    model, _, _ = oracle_model([([c["query"]], 0.0, 1.0)], c["reference"], dict(FIX["alignment_parameters"], MaxErrorRate=0.5))
    assert np.array_equal(model.depth[0], np.full(len(c["reference"]), UNIT, np.uint64))
    assert np.array_equal(counted(model).depth(0), np.ones(len(c["reference"])))
    # overlapping mates (mate 2 given as sequenced): one pair alignment of two sequences at 0 and 3, count 1 everywhere, also in the overlap 3..7
    c = FIX["match_database_cases"][1]
    q2 = api.decode(api.reverse_complement(api.encode(c["query2"])))
    model, alignments, _ = oracle_model([([c["query1"], q2], 0.0, 1.0)], c["reference"], dict(FIX["alignment_parameters"], MaxErrorRate=1.0))
    comps = alignments[0]
    assert len(comps) == 1 and len(comps[0]) == 1 and [sa.start_index_b() for sa in comps[0][0].components] == [c["start1"], c["start2"]]
    assert np.array_equal(model.depth[0], np.full(len(c["reference"]), UNIT, np.uint64))
    assert np.array_equal(counted(model).depth(0), np.ones(len(c["reference"])))


# ---------------------------------------------------------------- hand-written cases: the expected arrays are literals

def test_reversed_read_with_one_substitution():
    """Reference ACGTACGTAC; the aligned strand is reference[2:8] = GTACGT with its fourth base (reference 5, a C) read as A: GTAAGT.  The read is
    given as its reverse complement, ACTTAC."""
    ref = np.array([A, C_, G, T, A, C_, G, T, A, C_], np.uint8)
    given = np.array([A, C_, T, T, A, C_], np.uint8)  # reverse complement: G T A A G T
    model = PileupModel([("r", ref)])
    n = model.add([[[q_al(seq_al(0, True, [(0, 2, 6, 6)]))]]], [[given]])
    assert n == 0
    assert model.depth[0].tolist() == [0, 0, UNIT, UNIT, UNIT, UNIT, UNIT, UNIT, 0, 0]
    # reference[5] is C, the aligned strand holds A there: plane A, position 5
    assert model.alt[0].tolist() == [[0, 0, 0, 0, 0, UNIT, 0, 0, 0, 0], [0] * 10, [0] * 10, [0] * 10]
    assert model.middle[0].tolist() == model.depth[0].tolist()
    assert lines_of(counted(model)) == ["r\t6\tC\tA\t1\t1"]


def test_pair_overlapping_by_three_bases_with_an_odd_weight():
    """A pair with 32 alignments of which this is the first: weight 1441440 // 32 = 45045, odd, so the overlap splits it 22522 + 22523."""
    ref = np.array([A, C_, G, T] * 4, np.uint8)
    m1 = ref[1:8].copy()                                  # [1, 8)
    m2 = api.reverse_complement(ref[5:12])                # [5, 12), given as sequenced; overlap [5, 8)
    m1[5] = T                                             # reference[6] = G read as T by mate 1, inside the overlap
    w = UNIT // 32
    assert w == 45045 and UNIT % 32 == 0
    pair = q_al(seq_al(0, False, [(0, 1, 7, 7)]), seq_al(0, True, [(0, 5, 7, 7)]))
    far = [q_al(seq_al(1, False, [(0, 0, 7, 7)])) for _ in range(31)]  # the other 31 alignments lie on another contig
    model = PileupModel([("r", ref), ("other", np.full(8, N, np.uint8))])
    model.add([[[pair] + far]], [[m1, m2]])
    lo, hi = w // 2, w - w // 2
    assert (lo, hi) == (22522, 22523)
    assert model.depth[0].tolist() == [0, w, w, w, w, w, w, w, w, w, w, w, 0, 0, 0, 0]  # lo + hi = w in [5, 8)
    assert model.alt[0].tolist() == [[0] * 16, [0] * 16, [0] * 16, [0, 0, 0, 0, 0, 0, lo, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert model.depth[1].tolist() == [31 * w] * 7 + [0] and not model.alt[1].any()  # (an all-N contig: depth counts, alt does not)
    # the same with the substitution in mate 2: it adds the larger half
    m1[5] = G
    m2 = api.reverse_complement(np.concatenate([ref[5:6], [T], ref[7:12]]).astype(np.uint8))
    model = PileupModel([("r", ref), ("other", np.full(8, N, np.uint8))])
    model.add([[[pair] + far]], [[m1, m2]])
    assert model.alt[0][3].tolist() == [0, 0, 0, 0, 0, 0, hi, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_seventeen_alignments_share_one_read_exactly():
    ws = pileup_model.alignment_weights(17)
    assert UNIT % 17 == 10 and UNIT // 17 == 84790
    assert ws == [84791] * 10 + [84790] * 7 and sum(ws) == UNIT
    ref = np.tile(np.array([A, C_, G, T], np.uint8), 17)  # 17 windows of 4 bases
    read = np.array([A, C_, G, T], np.uint8)
    als = [q_al(seq_al(0, False, [(0, 4 * a, 4, 4)])) for a in range(17)]
    model = PileupModel([("r", ref)])
    model.add([[als]], [[read]])
    assert model.depth[0].tolist() == [84791] * 40 + [84790] * 28
    assert int(model.depth[0].sum()) == 4 * UNIT and not model.alt[0].any()
    for n in (2, 3, 5, 7, 11, 13, 16, 19, 23):
        ws = pileup_model.alignment_weights(n)
        assert sum(ws) == UNIT and ws == sorted(ws, reverse=True) and ws.count(ws[0]) in (n, UNIT % n)


def test_deletion_on_each_side_of_the_end_zone_boundary():
    """f = 0.1, len = 150: 0.1 * 150 is exactly 15.0 in doubles and 150 - 15.0 = 135.0, so k = 14 is the last base near the front end, k = 15 .. 134 are
    middle bases and k = 135 is the first base near the far end.  f = 0.07, len = 100 is where doubles show: 0.07 * 100 is 7.000000000000001, so
    k = 7 is still near the front end, and 100 - 7.000000000000001 = 93 after rounding, so k = 93 is near the far end."""
    assert 0.1 * 150 == 15.0 and 0.07 * 100 == 7.000000000000001 and 100 - 0.07 * 100 == 93.0
    assert pileup_model.near_query_end(np.arange(150), 150, 0.1).tolist() == [True] * 15 + [False] * 120 + [True] * 15
    assert pileup_model.near_query_end(np.arange(100), 100, 0.07).tolist() == [True] * 8 + [False] * 85 + [True] * 7
    assert not pileup_model.near_query_end(np.arange(150), 150, 0.0).any()
    rng = np.random.default_rng(5)
    ref = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, 400)]

    def deletion_at(k):  # a read of 150 bases whose 2-base deletion sits in front of query base k, from reference position 100
        read = np.concatenate([ref[100:100 + k], ref[102 + k:252]])
        blocks = [(0, 100, k, k), (k, 100 + k, 0, 2), (k, 102 + k, 150 - k, 150 - k)]
        model = PileupModel([("r", ref)], 0.1)
        model.add([[[q_al(seq_al(0, False, blocks))]]], [[read]])
        return model

    # query base j lies at reference 100 + j in front of the deletion and at 102 + j behind it; the middle bases are j = 15 .. 134
    for k, near, middle_from, middle_to in ((14, True, 117, 237),    # the deleted bases 114, 115 are near the end; 15 .. 134 lie at 117 .. 236
                                            (15, False, 115, 237),   # the deleted bases 115, 116 count, then 117 .. 236
                                            (134, False, 115, 237),  # 15 .. 133 at 115 .. 233, the deleted bases 234, 235, base 134 at 236
                                            (135, True, 115, 235)):  # 15 .. 134 at 115 .. 234; the deleted bases 235, 236 are near the end
        model = deletion_at(k)
        assert model.depth[0].tolist() == [0] * 100 + [UNIT] * 152 + [0] * 148
        assert model.middle[0].tolist() == [0] * middle_from + [UNIT] * (middle_to - middle_from) + [0] * (400 - middle_to), k
        assert model.events == [(0, 100 + k, 2, 2, 0, 4 if near else 0, k, UNIT)]
    # with fraction 0 the event has no flag and the middle depth is the depth
    model = PileupModel([("r", ref)], 0.0)
    model.add([[[q_al(seq_al(0, False, [(0, 100, 14, 14), (14, 114, 0, 2), (14, 116, 136, 136)]))]]], [[np.concatenate([ref[100:114], ref[116:252]])]])
    assert model.events == [(0, 114, 2, 2, 0, 0, 14, UNIT)] and np.array_equal(model.middle[0], model.depth[0])


def test_fallback_pair_reads_the_component_index_as_the_mate_and_ordinals_run_on():
    """Two components = the pair fell back to unpaired alignments: component 1's single sequence is mate 2.  Its insertion event carries mate bit 1,
    and the second batch's ordinals continue behind the first's."""
    ref = np.array([A, C_, G, T, T, G, C_, A, A, C_, G, G], np.uint8)
    junk = np.array([T, T, T, T], np.uint8)
    mate2 = np.array([A, C_, G, G, G, T, T, G], np.uint8)  # ACG + an inserted GG + TTG against reference[0:6] = ACGTTG
    fallback = [[], [q_al(seq_al(0, False, [(0, 0, 3, 3), (3, 3, 2, 0), (5, 3, 3, 3)]))]]
    model = PileupModel([("r", ref)])
    model.add([[[q_al(seq_al(0, False, [(0, 8, 4, 4)]))]]], [[ref[8:12]]])
    model.add([fallback], [[junk, mate2]])
    assert model.depth[0].tolist() == [UNIT] * 6 + [0, 0] + [UNIT] * 4 and not model.alt[0].any()
    assert model.events == [(0, 3, 1, 2, 1, 1, 3, UNIT)]
    m = counted(model, [[api.Query(ref[8:12])], [api.Query(junk, mate2)]])
    assert lines_of(m) == ["r\t3\t--\tGG\t1\t1"]


# ---------------------------------------------------------------- threshold logic of the host half on model-fed counts

def fed(ref_text, depth, alt=None, middle=None, events=(), batches=(), fraction=0.0):
    ref = api.encode(ref_text)
    n = len(ref)
    d = (np.asarray(depth, np.float64) * UNIT).round().astype(np.uint64)
    a = np.zeros((4, n), np.uint64)
    for (plane, pos), v in (alt or {}).items():
        a[plane, pos] = int(round(v * UNIT))
    m = d if middle is None else (np.asarray(middle, np.float64) * UNIT).round().astype(np.uint64)
    return pileup.CountedMatchDatabase([("r", ref)], [d], [a], [m], events, batches, fraction)


def test_float32_product_rule_keeps_a_support_of_seven_in_ten():
    """0.7 of a depth of 10 is 7.0 in float and 7.000000000000001 in double: an allele seen 7 times passes a fraction of 0.7, one seen 6 times does not."""
    assert np.float32(0.7) * np.float32(10) == np.float32(7)
    m = fed("ACGTACGT", [10] * 8, {(3, 2): 7, (0, 5): 6})
    assert lines_of(m) == ["r\t3\tG\tT\t7\t10", "r\t6\tC\tA\t6\t10"]
    assert lines_of(m, pileup.MutationDetectionParameters(minSNPDepthFraction=0.7)) == ["r\t3\tG\tT\t7\t10"]
    assert lines_of(m, pileup.MutationDetectionParameters(minSNPTotalDepth=10)) == ["r\t3\tG\tT\t7\t10", "r\t6\tC\tA\t6\t10"]
    assert lines_of(m, pileup.MutationDetectionParameters(minSNPTotalDepth=10.5)) == []
    # where float and double part: the float nearest 0.8 is 0.800000011920929, whose double product with 5 lies above 4 - in float it is 4.0, and 4 of 5 stay
    assert float(np.float32(0.8)) * 5 > 4 and np.float32(0.8) * np.float32(5) == np.float32(4)
    m5 = fed("ACGTACGT", [5] * 8, {(3, 2): 4, (0, 5): 3})
    assert lines_of(m5, pileup.MutationDetectionParameters(minSNPDepthFraction=0.8)) == ["r\t3\tG\tT\t4\t5"]
    # the same rule for an indel's start: a deletion supported by 7 of a middle depth of 10
    ev = [(0, 2, 2, 3, q, 0, 5, UNIT) for q in range(7)]
    m = fed("ACGTACGT", [10] * 8, events=ev)
    assert lines_of(m, pileup.MutationDetectionParameters(minIndelStartDepthFraction=0.7)) == ["r\t3\tGTA\t---\t7\t10"]
    assert lines_of(m, pileup.MutationDetectionParameters(minIndelStartDepthFraction=0.71)) == []


def test_continuation_cut_of_a_deletion():
    """A 4-base deletion at reference 2..5 with support 2: its start sees a middle depth of 2, base 3 one of 2, base 4 one of 4 - where 2 of 4 fails a
    continuation fraction of 0.7 - so the deletion is cut to its first two bases; a continuation total depth asked above what base 3 has cuts it to one."""
    ev = [(0, 2, 2, 4, 0, 0, 9, UNIT), (0, 2, 2, 4, 1, 0, 7, UNIT)]
    m = fed("ACGTACGT", [4] * 8, middle=[4, 4, 2, 2, 4, 4, 4, 4], events=ev)
    assert lines_of(m) == ["r\t3\tGTAC\t----\t2\t2"]
    assert lines_of(m, pileup.MutationDetectionParameters(minIndelContinuationDepthFraction=0.7)) == ["r\t3\tGT\t--\t2\t2"]
    assert lines_of(m, pileup.MutationDetectionParameters(minIndelContinuationTotalDepth=3)) == ["r\t3\tG\t-\t2\t2"]
    assert lines_of(m, pileup.MutationDetectionParameters(minIndelTotalStartDepth=3)) == []
    # an event near a query end (flag bit 2) supports nothing
    ev = [(0, 2, 2, 4, 0, 4, 9, UNIT), (0, 2, 2, 4, 1, 0, 7, UNIT)]
    m = fed("ACGTACGT", [4] * 8, middle=[4, 4, 2, 2, 4, 4, 4, 4], events=ev, fraction=0.1)
    assert lines_of(m) == ["r\t3\tGTAC\t----\t1\t2"]


def test_line_order_at_one_position():
    """At one position: substitutions first (by allele), then insertions, then deletions; an insertion is reported at the base before it (1-based
    position = startB), a deletion at its first base (startB + 1), so the insertion in front of reference base 3 and the substitution of base 2 share
    position 3 with the deletion of base 2."""
    read = api.Query(api.encode("ACTTG"))
    ev = [(0, 2, 2, 1, 0, 0, 2, UNIT),                 # deletion of reference base 2 -> position 3
          (0, 3, 1, 2, 1, 0, 2, UNIT)]                 # insertion of read[2:4] = TT in front of reference base 3 -> position 3
    m = fed("ACGTACGT", [3] * 8, {(3, 2): 1, (0, 2): 1, (0, 1): 1}, events=ev, batches=[[read, read]])
    assert lines_of(m) == ["r\t2\tC\tA\t1\t3", "r\t3\tG\tA\t1\t3", "r\t3\tG\tT\t1\t3", "r\t3\t--\tTT\t1\t3", "r\t3\tG\t-\t1\t3"]
    # without the reads an insertion is reported by its length
    m = fed("ACGTACGT", [3] * 8, events=ev[1:])
    assert lines_of(m) == ["r\t3\t--\tNN\t1\t3"]


# ---------------------------------------------------------------- the GPU tier's workloads, tried with the oracle

import pileup_workloads as W

WORKLOADS = ("several_contigs", "overlapping_pairs", "many_equal_alignments", "fallback_pairs", "ambiguous_reads_and_reference", "long_reads", "three_batches")


@pytest.mark.parametrize("name", WORKLOADS)
def test_workloads_hold_their_shapes_with_the_oracle(name):
    """The inputs of tests/test_gpu_pileup.py aligned by the oracle and recounted (the model asserts conservation on every batch): the shapes each workload
    exists for are there before a GPU sees it, and the end zone at fraction 0.1 has events on both sides and positions with a partial middle depth."""
    contigs, batches = getattr(W, name)()
    oracle = oracle_lib.OracleReference(contigs, mode="mapper")
    model = PileupModel(contigs, 0.1)
    alignments, mates = [], []
    for b in batches:
        st = oracle.align(b, oracle_lib.make_params(), threads=4)
        al = [api.decode_streams(st.ints, st.dbls, st.int_off, st.dbl_off, q) for q in range(b.nq)]
        model.add(al, W.mates_of(b))
        alignments += al
        mates += W.mates_of(b)
    flagged, unflagged, partial = W.end_zone_shapes(model.events, model.depth, model.middle)
    assert flagged > 0 and unflagged > 0 and partial > 0
    assert set(e[4] for e in model.events) <= set(q for q, comps in enumerate(alignments) if any(comps))
    if name == "several_contigs":
        assert all(d[0] > 0 and d[-1] > 0 and not d[u].any() for d, u in zip(model.depth, W.unreached(contigs)))
    if name == "overlapping_pairs":
        lengths, indels_inside, odd = W.overlaps(alignments)
        assert {100, 60, 30, 1} <= lengths and indels_inside > 0 and odd > 0
    if name == "many_equal_alignments":
        assert set(W.FAMILY_SIZES) <= W.alignment_counts(alignments)
    if name == "fallback_pairs":
        assert W.fallback_shapes(alignments, mates, contigs) == {(c, s) for c in range(3) for s in ((1, 0), (0, 1))}
        assert all(d[0] > 0 and d[-1] > 0 for d in model.depth)
    if name == "ambiguous_reads_and_reference":
        in_read, in_ref = W.ambiguous_positions(alignments, mates, contigs)
        assert in_read >= 100 and in_ref >= 100
    if name == "three_batches":
        assert [b.nq for b in batches] == [700, 40, 1] and not any(any(c) for c in alignments[700:740]) and any(e[4] == 740 for e in model.events)
