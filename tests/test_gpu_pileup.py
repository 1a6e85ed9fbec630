"""the pile-up of alignments on the reference (device) and the mutations file (host), against what the
reference's own tests pin - tests/golden/mutations_reference.json transcribes src/test/java/MutationsWriter_Test.java:18-134 and
src/test/java/MatchDatabase_Test.java:12-69 (inputs and expected values)."""
import io
import json
import os
import numpy as np
import pytest

from mapper_amd import api, pileup, synth, multi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "mutations_reference.json")))


def build(query_texts, reference, params=None, query_end_fraction=0.0):
    db = api.ReferenceDatabase([("ref", reference)], mode="api")
    queries = [api.Query(*[api.encode(t) for t in qt]) if isinstance(qt, (list, tuple)) else api.Query(api.encode(qt)) for qt in query_texts]
    r = db.align_batch(queries, api.AlignmentParameters(**(params or FIX["alignment_parameters"])))
    m = pileup.MatchDatabase(db, query_end_fraction)
    m.add_last(queries)
    return db, m, r


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIX["mutation_cases"], ids=[c["name"] for c in FIX["mutation_cases"]])
def test_mutations_writer_cases(case):
    db, m, _ = build([case["query"]], case["reference"], query_end_fraction=case.get("query_end_fraction", 0.0))
    out = io.StringIO()
    m.write_mutations(out, pileup.MutationDetectionParameters(**case.get("filter", {})))
    lines = [l for l in out.getvalue().split("\n") if l and not l.startswith("#") and not l.startswith("CHR")]  # (withoutMetadataLines, MutationsWriter_Test.java:144-154)
    assert lines == case["expected"]
    m.close(); db.close()


@pytest.mark.gpu
def test_match_database_counts():
    c = FIX["match_database_cases"][0]
    db, m, _ = build([c["query"]], c["reference"], dict(FIX["alignment_parameters"], MaxErrorRate=0.5))
    assert np.array_equal(m.depth(0), np.ones(len(c["reference"])))
    m.close(); db.close()
    # overlapping mates: mate 2 is given as sequenced (reverse complement), the pair overlaps on reference positions 3..7
    c = FIX["match_database_cases"][1]
    ref = c["reference"] * 1
    q1, q2 = c["query1"], api.decode(api.reverse_complement(api.encode(c["query2"])))
    db = api.ReferenceDatabase([("ref", ref)], mode="api")
    q = api.Query(api.encode(q1), api.encode(q2), expected_inner_distance=0.0, spacing_deviation_per_unit_penalty=1.0)
    r = db.align_batch([q], api.AlignmentParameters(**dict(FIX["alignment_parameters"], MaxErrorRate=1.0)))
    comps = r.query_alignments(0)
    # the aligner returns the pair as the reference's test builds it (MatchDatabase_Test.java:47-54): one alignment of two sequences at 0 and 3
    assert len(comps) == 1 and len(comps[0]) == 1 and [sa.start_index_b() for sa in comps[0][0].components] == [c["start1"], c["start2"]]
    m = pileup.MatchDatabase(db)
    m.add_last([q])
    assert np.array_equal(m.depth(0), np.ones(len(ref)))
    m.close()
    db.close()


@pytest.mark.gpu
def test_query_ends_and_thresholds_on_a_synthetic_batch():
    """--distinguish-query-ends 0.1 with the reference's default thresholds (Mapper.java:76,534-542) on a deep synthetic pile-up: the middle depth is
    the depth minus what the first and last tenth of every read contribute (recounted on the host), indels near read ends do not count, and the
    thresholds only ever remove lines."""
    ref = synth.synthetic_reference(20_000, seed=91)
    reads = synth.synthetic_single_end(ref, 3000, seed=92, indel_prob=0.3)[0]
    queries = [api.Query(r) for r in reads]
    db = api.ReferenceDatabase([("r", ref)])
    res = db.align_batch(queries, api.AlignmentParameters())
    m0 = pileup.MatchDatabase(db)
    m0.add_last(queries)
    m1 = pileup.MatchDatabase(db, 0.1)
    m1.add_last(queries)
    assert np.array_equal(m0._sum(0)[0], m1._sum(0)[0]) and np.array_equal(m0._middle(0), m0._sum(0)[0])
    mid = np.zeros(len(ref))
    for q in range(len(queries)):
        for comp in res.query_alignments(q):
            for al in comp:
                for sa in al.components:
                    for b in sa.sections:
                        n = len(reads[q])
                        ks = np.arange(b.startA, b.startA + b.lengthA) if b.lengthA == b.lengthB else np.full(b.lengthB, b.startA)
                        inner = ~((ks < 0.1 * n) | (ks >= n - 0.1 * n))
                        np.add.at(mid, b.startB + np.arange(len(ks))[inner], 1.0 / len(comp))
    assert np.allclose(m1._middle(0) / pileup.UNIT, mid, atol=1e-9)
    everything = m1.mutations(pileup.MutationDetectionParameters.emptyFilter())
    # (the defaults - 90 % of a depth of 5 and more - are a variant caller's: sequencing errors of a deep pile-up do not pass them)
    assert m1.mutations(pileup.MutationDetectionParameters.defaultFilter()) == []
    filtered = m1.mutations(pileup.MutationDetectionParameters(5.0, 0.08, 1.0, 0.08, 1.0, 0.08))
    assert 0 < len(filtered) < len(everything) and set((c, p) for c, p, *_ in filtered) <= set((c, p) for c, p, *_ in everything)
    assert len([x for x in everything if "-" in x[2] + x[3]]) < len([x for x in m0.mutations() if "-" in x[2] + x[3]])  # indels near read ends are gone
    m0.close(); m1.close(); db.close()


@pytest.mark.gpu
def test_pileup_on_a_synthetic_batch_and_two_replicas():
    """Depth and substitution counts of a few thousand reads equal a host recount from the decoded alignments; two replicas (batches dealt
    between them) sum to the same pile-up as one."""
    ref = synth.synthetic_reference(150_000, seed=61)
    reads = synth.synthetic_single_end(ref, 4000, seed=62, indel_prob=0.3)[0]
    queries = [api.Query(r) for r in reads]
    params = api.AlignmentParameters()
    db = api.ReferenceDatabase([("r", ref)])
    res = db.align_batch(queries, params)
    m = pileup.MatchDatabase(db)
    n_events = m.add_last(queries)
    depth = np.zeros(len(ref))
    alt = np.zeros((4, len(ref)))
    events = 0
    for q in range(len(queries)):
        comps = res.query_alignments(q)
        for comp in comps:
            for al in comp:
                w = 1.0 / len(comp)
                for sa in al.components:
                    qq = api.reverse_complement(reads[q]) if sa.reference_reversed else reads[q]
                    for b in sa.sections:
                        if b.lengthA == b.lengthB:
                            depth[b.startB:b.startB + b.lengthB] += w
                            for i in range(b.lengthA):
                                if qq[b.startA + i] != ref[b.startB + i]:
                                    alt[{1: 0, 2: 1, 4: 2, 8: 3}[int(qq[b.startA + i])], b.startB + i] += w
                        else:
                            events += 1
                            if b.lengthA == 0:
                                depth[b.startB:b.startB + b.lengthB] += w
    assert n_events == events and events > 500
    got_depth, got_alt = m._sum(0)
    assert np.allclose(got_depth / pileup.UNIT, depth, atol=1e-9) and np.allclose(got_alt / pileup.UNIT, alt, atol=1e-9)
    muts = m.mutations()
    assert len(muts) > 1000 and all(c == 0 and 1 <= p <= len(ref) for c, p, *_ in muts)
    # the same through two replicas
    two = multi.MultiGpuDatabase([("r", ref)], [0, 0])
    m2 = pileup.MatchDatabase(two.replicas)
    half = len(queries) // 2
    for rep, qs in ((0, queries[:half]), (1, queries[half:])):
        two.replicas[rep].align_batch(qs, params)
        m2.add_last(qs, replica=rep)
    d2, a2 = m2._sum(0)
    assert np.array_equal(d2, got_depth) and np.array_equal(a2, got_alt)
    assert m2.mutations() == muts
    m.close(); m2.close(); db.close(); two.close()


@pytest.mark.gpu
def test_cli_out_mutations(tmp_path):
    """`--out-mutations` (Mapper.java:187,758-785) through the command line, one GPU and two contexts, small batches: the same file."""
    from mapper_amd import cli
    ref = synth.synthetic_reference(80_000, seed=71)
    reads = synth.synthetic_single_end(ref, 900, seed=72, indel_prob=0.3)[0]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(ref) + "\n")
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
    outs = []
    for extra in ([], ["--devices", "0,0", "--batch-size", "128"]):
        path = tmp_path / ("mut%d.txt" % len(outs))
        assert cli.run(["--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--distinguish-query-ends", "0", "--out-mutations", str(path),
                        "--snp-threshold", "0", "0", "--indel-threshold", "0", "0"] + extra, out=io.StringIO()) == 0
        outs.append(open(path).read())
    assert outs[0] == outs[1]
    body = [l.split("\t") for l in outs[0].split("\n") if l and not l.startswith("#") and not l.startswith("CHR")]
    assert len(body) > 500 and all(l[0] == "chrSyn" and len(l) == 6 for l in body)
    assert any(set(l[2]) == {"-"} for l in body) and any(set(l[3]) == {"-"} for l in body)  # insertions and deletions are there


@pytest.mark.gpu
def test_cli_out_refs_map_count(tmp_path):
    """`--out-refs-map-count` (Mapper.java:197,747-756): reads from two contigs are counted under the contig they map to ([unpinned] file format)."""
    from mapper_amd import cli
    a, b = synth.synthetic_reference(60_000, seed=81), synth.synthetic_reference(40_000, seed=82)
    ra, rb = synth.synthetic_single_end(a, 300, seed=83)[0], synth.synthetic_single_end(b, 200, seed=84)[0]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrA\n" + api.decode(a) + "\n>chrB\n" + api.decode(b) + "\n")
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, r in enumerate(list(ra) + list(rb)):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
    assert cli.run(["--reference", str(tmp_path / "ref.fasta"), "--queries", str(tmp_path / "reads.fastq"), "--out-refs-map-count", str(tmp_path / "counts.txt")], out=io.StringIO()) == 0
    counts = dict(l.split("\t") for l in open(tmp_path / "counts.txt").read().split("\n") if l)
    assert int(counts["chrA"]) >= 295 and int(counts["chrB"]) >= 195 and sum(int(v) for v in counts.values()) <= 500


# ---------------------------------------------------------------- device counts against the plain recount (tests/pileup_model.py), exactly
# The kernel's sums are integers by design, so every comparison below is equality: np.array_equal on the units of depth, alt and middle, list
# equality on the events.  Each workload (tests/pileup_workloads.py) is piled up with fraction 0 and with a fraction > 0, and each test first asserts,
# on the GPU's own alignments and counts, that the shapes the workload exists for are there.

import oracle_lib
import pileup_workloads as W
from pileup_model import PileupModel, event_order


def device_counts(m, contigs):
    """depth, alt, middle per contig and the events (eight fields each) of a one-replica MatchDatabase."""
    sums = [m._sum(c) for c in range(len(contigs))]
    return [s[0] for s in sums], [s[1] for s in sums], [m._middle(c) for c in range(len(contigs))], [e[1:] for e in m._events()]


def assert_equals_model(m, model, contigs):
    depth, alt, middle, events = device_counts(m, contigs)
    for c in range(len(contigs)):
        assert np.array_equal(depth[c], model.depth[c]), "depth of contig %d differs first at %d" % (c, int(np.nonzero(depth[c] != model.depth[c])[0][0]))
        assert np.array_equal(alt[c], model.alt[c]), "alt of contig %d differs first at (plane, position) %r" % (c, tuple(int(x[0]) for x in np.nonzero(alt[c] != model.alt[c])))
        assert np.array_equal(middle[c], model.middle[c]), "middle depth of contig %d differs first at %d" % (c, int(np.nonzero(middle[c] != model.middle[c])[0][0]))
    assert all(event_order(a) <= event_order(b) for a, b in zip(events, events[1:]))  # the order xm_pileup_add_last documents
    assert sorted(events, key=event_order) == model.sorted_events()
    # and the host half says the same of both (event grouping, insertion texts, line order)
    fed = pileup.CountedMatchDatabase(model.contigs, model.depth, model.alt, model.middle, model.sorted_events(), m._batches[0], model.f)
    assert m.mutations() == fed.mutations()
    return depth, alt, middle, events


def pile_up(contigs, batches, fractions):
    """Aligns the batches on the GPU and adds each, while it is resident, to one device pile-up and one model per fraction."""
    db = api.ReferenceDatabase(contigs)
    ms = [pileup.MatchDatabase(db, f) for f in fractions]
    models = [PileupModel(contigs, f) for f in fractions]
    alignments, mates = [], []
    for b in batches:
        res = db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())
        al, mt = [res.query_alignments(q) for q in range(b.nq)], W.mates_of(b)
        for m, model in zip(ms, models):
            assert m.add_last(mt) == model.add(al, mt)  # (num_events is the running total)
        alignments += al
        mates += mt
    return db, ms, models, alignments, mates


def compare_workload(contigs, batches, fractions=(0.0, 0.1)):
    db, ms, models, alignments, mates = pile_up(contigs, batches, fractions)
    counts = []
    for m, model in zip(ms, models):
        depth, alt, middle, events = assert_equals_model(m, model, contigs)
        if model.f > 0:  # the end zone is there: events on both sides of it, positions whose middle depth is a part of the depth
            flagged, unflagged, partial = W.end_zone_shapes(events, depth, middle)
            assert flagged > 0 and unflagged > 0 and partial > 0, (model.f, flagged, unflagged, partial)
        else:
            assert all(np.array_equal(d, x) for d, x in zip(depth, middle)) and not any(e[5] & 4 for e in events)
        counts.append((depth, alt, middle, events))
    for c in range(len(contigs)):  # the fraction changes the middle depth and the flags only
        assert all(np.array_equal(counts[0][0][c], k[0][c]) and np.array_equal(counts[0][1][c], k[1][c]) for k in counts[1:])
    return db, ms, models, alignments, mates, counts


def close_all(db, ms):
    for m in ms:
        m.close()
    db.close()


@pytest.mark.gpu
def test_device_pileup_equals_the_model_on_several_contigs():
    """Workload a: contigStart > 0 and an alt plane stride that is not the contig's length; the first and the last base of every contig covered;
    fractions 0, 0.1 and 0.37; ranges read with first > 0 and n < len."""
    contigs, batches = W.several_contigs()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches, (0.0, 0.1, 0.37))
    depth, alt, middle, events = counts[0]
    assert set(sa.contig for *_, sa in W.sequence_alignments(alignments)) == {0, 1, 2}
    assert set(e[0] for e in events) == {0, 1, 2} and set(e[2] for e in events) == {1, 2} and set((e[5] >> 1) & 1 for e in events) == {0, 1}
    for c, reach in enumerate(W.unreached(contigs)):
        assert depth[c][0] > 0 and depth[c][-1] > 0 and alt[c].any()
        for k in counts:  # what no read reaches stays 0 in every array, on both sides of every contig boundary
            assert not k[0][c][reach].any() and not k[1][c][:, reach].any() and not k[2][c][reach].any()
        assert reach[150] and reach[len(reach) - 151] and depth[c][149] > 0 and depth[c][len(reach) - 150] > 0
    # pieces of contigs through the C entries themselves
    L = ms[1]._L
    for c, (_, ref) in enumerate(contigs):
        n = len(ref)
        for first, count in ((1, n - 1), (n - 1, 1), (137, 1000), (n - 1000, 999), (0, 1), (n // 2, 0)):
            d = np.full(count + 1, 7, np.uint64); a = np.full((4, count + 1), 7, np.uint64)[:, :count].copy(); mid = np.full(count + 1, 7, np.uint64)
            assert L.xm_pileup_read(ms[1]._h[0], c, first, count, d.ctypes.data, a.ctypes.data) == 0
            assert L.xm_pileup_read_middle(ms[1]._h[0], c, first, count, mid.ctypes.data) == 0
            assert np.array_equal(d[:count], models[1].depth[c][first:first + count]) and d[count] == 7 and mid[count] == 7
            assert np.array_equal(a, models[1].alt[c][:, first:first + count]) and np.array_equal(mid[:count], models[1].middle[c][first:first + count])
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_on_overlapping_pairs():
    """Workload b: pair alignments whose two sequences share reference bases - w // 2 from the first, w - w // 2 from the second, odd weights included."""
    contigs, batches = W.overlapping_pairs()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    lengths, indels_inside, odd = W.overlaps(alignments)
    assert {100, 60, 30, 1} <= lengths and indels_inside > 0 and odd > 0, (sorted(lengths), indels_inside, odd)
    assert {17, 19} <= W.alignment_counts(alignments)
    assert set((e[5] & 1, (e[5] >> 1) & 1) for e in counts[0][3]) == {(0, 0), (0, 1), (1, 0), (1, 1)}  # indels of both mates on both strands
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_on_queries_with_many_equal_alignments():
    """Workload c: n alignments share one read exactly - UNIT // n each, the first UNIT % n one unit more - for every n of the list, 17, 19 and 23 among
    them, with pairs from inside the families."""
    contigs, batches = W.many_equal_alignments()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    assert set(W.FAMILY_SIZES) <= W.alignment_counts(alignments), sorted(W.alignment_counts(alignments))
    lengths, indels_inside, odd = W.overlaps(alignments)
    assert odd > 0 and len(lengths) > 0
    weights = set(e[7] for e in counts[0][3])
    assert {pileup.UNIT // 17, pileup.UNIT // 17 + 1, pileup.UNIT // 23, pileup.UNIT // 23 + 1} <= weights  # events on both sides of the remainder rule
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_on_pairs_that_fall_back_to_unpaired_alignments():
    """Workload d: two components of which one is empty - component c's sequence is mate c, whichever index it has in its alignment."""
    contigs, batches = W.fallback_pairs()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    found = W.fallback_shapes(alignments, mates, contigs)
    assert found == {(c, shape) for c in range(len(contigs)) for shape in ((1, 0), (0, 1))}, sorted(found)
    depth, alt, middle, events = counts[0]
    for c in range(len(contigs)):
        assert depth[c][0] > 0 and depth[c][-1] > 0 and alt[c].any()
    # an indel of a lone mate 2 carries the mate bit
    lone_second = set(q for q, comps in enumerate(alignments) if len(comps) == 2 and not comps[0] and comps[1])
    assert any(e[4] in lone_second and e[5] & 1 for e in events) and all(e[5] & 1 for e in events if e[4] in lone_second)
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_with_ambiguity_codes():
    """Workload e: depth counts and alt does not, at ambiguous read bases and at ambiguous reference bases alike."""
    contigs, batches = W.ambiguous_reads_and_reference()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    in_read, in_ref = W.ambiguous_positions(alignments, mates, contigs)
    assert in_read >= 100 and in_ref >= 100, (in_read, in_ref)
    depth, alt, middle, events = counts[0]
    for c, (_, ref) in enumerate(contigs):
        ambiguous = ~np.isin(ref, [1, 2, 4, 8])
        assert depth[c][ambiguous].any() and not alt[c][:, ambiguous].any()
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_on_long_reads():
    """Workload f: 1 kb reads - dozens of blocks and events per query, deletions on both sides of the end zone."""
    contigs, batches = W.long_reads()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    events = counts[1][3]
    per_query = np.bincount([e[4] for e in events])
    assert len(alignments) >= 300 and sum(1 for c in alignments if any(c)) >= 250 and per_query.max() >= 6
    assert any(e[2] == 2 and e[5] & 4 for e in events) and any(e[2] == 2 and not e[5] & 4 for e in events)
    close_all(db, ms)


@pytest.mark.gpu
def test_device_pileup_equals_the_model_over_three_batches():
    """Workload g: three add_last calls - 700 queries, 40 of which none aligns, one query: ordinals run on across the calls, num_events is the running
    total, and xm_pileup_events paged by a small n returns what one large read returns."""
    contigs, batches = W.three_batches()
    db, ms, models, alignments, mates, counts = compare_workload(contigs, batches)
    sizes = [b.nq for b in batches]
    assert sizes == [700, 40, 1]
    assert not any(any(c) for c in alignments[700:740]) and any(alignments[740])
    events = counts[0][3]
    assert any(e[4] == 740 for e in events) and any(e[4] < 700 for e in events) and not any(700 <= e[4] < 740 for e in events)
    L, h = ms[0]._L, ms[0]._h[0]
    whole = np.zeros((len(events) + 5, 8), np.int64)
    assert L.xm_pileup_events(h, 0, len(whole), whole.ctypes.data) == len(events)
    assert [tuple(int(x) for x in r) for r in whole[:len(events)]] == events
    paged, page = [], np.zeros((7, 8), np.int64)
    while True:
        got = L.xm_pileup_events(h, len(paged), 7, page.ctypes.data)
        assert 0 <= got <= 7
        if got == 0:
            break
        paged += [tuple(int(x) for x in r) for r in page[:got]]
    assert paged == events
    close_all(db, ms)


# ---------------------------------------------------------------- the error contract of the pile-up entries

def small_batch(seed=5):
    ref = synth.synthetic_reference(6_000, seed=seed)
    return [("long", ref), ("short", synth.synthetic_reference(2_000, seed=seed + 1))], oracle_lib.QueryBatch(W.noisy_reads(ref, 64, seed + 2))


def align(db, b):
    return db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())


@pytest.mark.gpu
def test_set_query_ends_refuses_bad_fractions_and_calls_after_the_first_add():
    contigs, b = small_batch()
    db = api.ReferenceDatabase(contigs)
    with pytest.raises(RuntimeError, match="must be >= 0 and < 1"):
        pileup.MatchDatabase(db, 1.0)
    m = pileup.MatchDatabase(db, 0.0)
    L, h = m._L, m._h[0]
    for bad in (-0.1, -1e-300, 1.0, 1.5, float("nan"), float("inf")):
        assert L.xm_pileup_set_query_ends(h, bad) != 0 and b"must be >= 0 and < 1" in L.xm_last_error(), bad
    assert L.xm_pileup_set_query_ends(h, 0.25) == 0 and L.xm_pileup_set_query_ends(h, 0.999) == 0 and L.xm_pileup_set_query_ends(h, 0.1) == 0  # (before the first add: any number of times)
    align(db, b)
    m.add_last()
    assert L.xm_pileup_set_query_ends(h, 0.2) != 0 and b"already added" in L.xm_last_error()
    assert L.xm_pileup_set_query_ends(h, 0.0) != 0
    assert L.xm_pileup_set_query_ends(None, 0.1) != 0
    m.close(); db.close()


@pytest.mark.gpu
def test_pileup_reads_refuse_ranges_outside_the_contig_and_accept_none():
    contigs, b = small_batch()
    db = api.ReferenceDatabase(contigs)
    m = pileup.MatchDatabase(db, 0.1)
    align(db, b)
    m.add_last()
    L, h = m._L, m._h[0]
    d = np.zeros(8_000, np.uint64); a = np.zeros((4, 8_000), np.uint64)
    for contig, first, n in ((0, 0, 6_001), (0, 1, 6_000), (0, 6_000, 1), (1, 0, 2_001), (1, 1_999, 2), (0, -1, 10), (0, 10, -1), (-1, 0, 10), (2, 0, 10), (1, 2_001, 0)):
        assert L.xm_pileup_read(h, contig, first, n, d.ctypes.data, a.ctypes.data) != 0 and b"range outside of the contig" in L.xm_last_error(), (contig, first, n)
        assert L.xm_pileup_read_middle(h, contig, first, n, d.ctypes.data) != 0 and b"range outside of the contig" in L.xm_last_error(), (contig, first, n)
    assert not d.any() and not a.any()  # a refused read writes nothing
    for contig, first in ((0, 0), (0, 6_000), (1, 2_000), (1, 77)):  # n == 0 is a range, also at the contig's end
        assert L.xm_pileup_read(h, contig, first, 0, d.ctypes.data, a.ctypes.data) == 0 and L.xm_pileup_read_middle(h, contig, first, 0, d.ctypes.data) == 0
    assert L.xm_pileup_read(h, 1, 0, 2_000, d.ctypes.data, a.ctypes.data) == 0 and L.xm_pileup_read_middle(h, 1, 1_999, 1, d.ctypes.data) == 0  # the whole contig, its last base
    assert L.xm_pileup_read(h, 0, 0, 10, None, a.ctypes.data) != 0 and L.xm_pileup_read_middle(h, 0, 0, 10, None) != 0
    m.close(); db.close()


@pytest.mark.gpu
def test_add_last_needs_the_batch_of_the_last_align_call_resident():
    contigs, b = small_batch()
    arrays = (b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation)
    message = "the batch of the last align call is no longer resident"
    db = api.ReferenceDatabase(contigs)
    m = pileup.MatchDatabase(db)
    with pytest.raises(RuntimeError, match=message):  # nothing was aligned yet
        m.add_last()
    align(db, b)
    n = m.add_last()
    assert n > 0
    db.upload_arrays(*arrays)                         # the next batch is uploaded: the streams no longer belong to the resident batch
    with pytest.raises(RuntimeError, match=message):
        m.add_last()
    db.align_resident(api.AlignmentParameters())
    assert m.add_last() == 2 * n
    db.stage_arrays(*arrays)                          # staged only: the resident batch is untouched (the next batch is copied while this one is piled up)
    assert m.add_last() == 3 * n
    db.commit_staged()                                # committed: the staged batch is the resident one now
    with pytest.raises(RuntimeError, match=message):
        m.add_last()
    assert m._L.xm_pileup_add_last(None, None) != 0
    depth = m._sum(0)[0]
    one = pileup.MatchDatabase(db)
    db.align_resident(api.AlignmentParameters())
    one.add_last()
    assert np.array_equal(depth, 3 * one._sum(0)[0])   # the refused calls added nothing
    m.close(); one.close(); db.close()


@pytest.mark.gpu
def test_pileup_events_paging_limits_and_life_after_the_context():
    """xm_pileup_events returns -1 for a first beyond the end (0 at the end); a pile-up is read and freed after its context was closed."""
    contigs, b = small_batch()
    db = api.ReferenceDatabase(contigs)
    m = pileup.MatchDatabase(db, 0.1)
    res = align(db, b)
    n = m.add_last()
    model = PileupModel(contigs, 0.1)
    model.add([res.query_alignments(q) for q in range(b.nq)], W.mates_of(b))
    assert n == len(model.events) and n > 0
    L, h = m._L, m._h[0]
    buf = np.zeros((n + 1, 8), np.int64)
    assert L.xm_pileup_events(h, n, 4, buf.ctypes.data) == 0 and L.xm_pileup_events(h, n + 1, 4, buf.ctypes.data) == -1 and L.xm_pileup_events(h, -1, 4, buf.ctypes.data) == -1
    assert L.xm_pileup_events(h, 0, 0, None) == 0 and L.xm_pileup_events(h, 0, 4, None) == -1 and L.xm_pileup_events(None, 0, 4, buf.ctypes.data) == -1
    assert L.xm_pileup_events(h, n - 1, 4, buf.ctypes.data) == 1 and not buf[1:].any()
    db.close()                                         # the context goes first
    depth, alt, middle, events = device_counts(m, contigs)
    for c in range(len(contigs)):
        assert np.array_equal(depth[c], model.depth[c]) and np.array_equal(alt[c], model.alt[c]) and np.array_equal(middle[c], model.middle[c])
    assert events == model.sorted_events()
    m.close()
