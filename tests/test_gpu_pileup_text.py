"""The text of insertions kept in the device pile-up (xm_pileup_keep_insert_text, xm_pileup_event_text): every insertion event's device text
against the text the host derives from the queries (the definition: pileup.MatchDatabase.mutations), over real batches, several batches and replicas,
ambiguity codes, the edge shapes of the three stages through xm_test_pileup_text, the contract of the entries, and the command line, whose --out-mutations
jobs now stream and must write byte for byte what the per-object path writes."""
import ctypes as C
import io

import numpy as np
import pytest

import oracle_lib
import pileup_text_cases as tc
import pileup_workloads as W
from mapper_amd import _capi, api, cli, multi, pileup, synth

PARAMS = api.AlignmentParameters


def align(db, b):
    return db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, PARAMS())


def events_and_texts(m):
    """The events of a one-replica MatchDatabase (eight fields each) and, per event, the text the device kept (None for a deletion)."""
    events = [e[1:] for e in m._events()]
    return events, [m._texts.get((0, k)) for k in range(len(events))]


def page_text(L, h, first, n, cap):
    """xm_pileup_event_text into buffers with guard bytes -> (m, offsets[m + 1], text) or (-1, None, None)."""
    off = np.full(max(n, 0) + 2, -7, np.int64)
    text = np.full(cap + 8, 0x7E, np.uint8)
    m = L.xm_pileup_event_text(h, first, n, off.ctypes.data, text.ctypes.data, cap)
    if m < 0:
        return m, None, None
    assert off[0] == 0 and off[m] <= cap and np.all(np.diff(off[:m + 1]) >= 0) and off[m + 1] == -7 and np.all(text[off[m]:] == 0x7E)   # nothing behind what was served
    return m, off[:m + 1].copy(), text[:off[m]].tobytes()


# ---------------------------------------------------------------- 1. real batches

def single_end_workload():
    ref = synth.synthetic_reference(20_000, seed=91)
    reads = synth.synthetic_single_end(ref, 3000, seed=92, indel_prob=0.3)[0]
    return [("r", ref)], oracle_lib.QueryBatch([W.single(r) for r in reads])


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["single_end", "pairs"])
def test_device_text_equals_the_text_derived_from_the_queries(workload):
    contigs, b = single_end_workload() if workload == "single_end" else tc.pairs_with_insertions()
    mates = W.mates_of(b)
    db = api.ReferenceDatabase(contigs)
    res = align(db, b)
    seen = []
    for fraction in (0.0, 0.1):
        m = pileup.MatchDatabase(db, fraction, keep_insert_text=True)
        n = m.add_last(None)
        events, texts = events_and_texts(m)
        insertions = [e for e in events if e[2] == 1]
        # the shapes are there, on the GPU's own events: insertions of reversed alignments, and for pairs insertions in mate 2 and of queries with several alignments
        assert n == len(events) and len(insertions) > 300 and sum(1 for e in insertions if e[5] & 2) > 100 and sum(1 for e in insertions if not e[5] & 2) > 100
        if workload == "pairs":
            assert sum(1 for e in insertions if e[5] & 1) > 100 and sum(1 for e in insertions if not e[5] & 1) > 100
            several = set(q for q in set(e[4] for e in insertions) if any(len(comp) >= 2 for comp in res.query_alignments(q)))
            assert len(several) >= 10
            assert any(sum(1 for e in insertions if e[4] == q) >= 2 for q in several)
        assert (fraction > 0) == any(e[5] & 4 for e in events)
        want = tc.insertion_texts(events, lambda ordinal: mates[ordinal])
        assert texts == want
        assert all(len(t) == e[3] and set(t) <= set("ACGT") for e, t in zip(events, texts) if t is not None)
        seen.append((events, texts))
        m.close()
    assert [t for t in seen[0][1]] == [t for t in seen[1][1]]   # the fraction changes the flags only
    db.close()


# ---------------------------------------------------------------- 2. several batches into one pile-up, and two replicas

def three_batches_with_insertions(seed=0x3B3):
    rng = np.random.default_rng(seed)
    contigs = [("c%d" % i, synth.synthetic_reference(n, seed=seed + i)) for i, n in enumerate((8_000, 5_000, 2_500))]
    first = []
    for c, (_, ref) in enumerate(contigs):
        first += W.noisy_reads(ref, (400, 200, 100)[c], seed + 8 + c, indel_prob=0.5)
    junk = [W.single(W.CODES[rng.integers(0, 4, 150)]) for _ in range(40)]
    last = W.noisy_reads(contigs[1][1], 60, seed + 16, indel_prob=0.9)
    return contigs, [oracle_lib.QueryBatch(first), oracle_lib.QueryBatch(junk), oracle_lib.QueryBatch(last)]


@pytest.mark.gpu
def test_three_batches_into_one_pileup_and_two_replicas():
    """An event of the third batch reads the third batch's bases (the ordinal runs on, the bases are the resident batch's); the mutations with kept text
    and no queries equal the mutations of a pile-up that was handed the queries, through one context and through two replicas."""
    contigs, batches = three_batches_with_insertions()
    db = api.ReferenceDatabase(contigs)
    kept, fed = pileup.MatchDatabase(db, 0.1, keep_insert_text=True), pileup.MatchDatabase(db, 0.1)
    mates = []
    for b in batches:
        align(db, b)
        assert kept.add_last(None) == fed.add_last(W.mates_of(b))
        mates += W.mates_of(b)
    events, texts = events_and_texts(kept)
    assert sum(1 for e in events if e[2] == 1 and e[4] >= 740) >= 5 and sum(1 for e in events if e[2] == 1 and e[4] < 700) >= 100 and not any(700 <= e[4] < 740 for e in events)
    assert texts == tc.insertion_texts(events, lambda ordinal: mates[ordinal])
    want = fed.mutations()
    insertions = [row for row in want if set(row[2]) == {"-"}]
    assert len(insertions) > 50 and all(set(row[3]) <= set("ACGT") for row in insertions)
    assert kept.mutations() == want
    two = multi.MultiGpuDatabase(contigs, [0, 0])
    m2 = pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True)
    for rep, b in ((0, batches[0]), (1, batches[1]), (1, batches[2])):
        align(two.replicas[rep], b)
        m2.add_last(None, replica=rep)
    assert m2.mutations() == want
    kept.close(); fed.close(); m2.close(); db.close(); two.close()


# ---------------------------------------------------------------- 3. ambiguity codes inside an insertion

@pytest.mark.gpu
def test_ambiguity_codes_inside_an_insertion_come_through_the_table():
    ref = synth.synthetic_reference(6_000, seed=33)
    reads = tc.reads_with_ambiguous_insertions(ref, 40, seed=34)
    b = oracle_lib.QueryBatch([W.single(r) for r in reads])
    db = api.ReferenceDatabase([("r", ref)])
    align(db, b)
    m = pileup.MatchDatabase(db, keep_insert_text=True)
    m.add_last(None)
    events, texts = events_and_texts(m)
    inserted = [t for t in texts if t is not None]
    assert texts == tc.insertion_texts(events, lambda ordinal: [reads[ordinal]])
    ambiguous = lambda t: t is not None and bool(set(t) & set("NR"))  # noqa: E731  (where the aligner puts the gap decides whether a neighbour comes with it)
    assert sum(1 for t in inserted if ambiguous(t)) >= 30 and "NR" in inserted
    assert any(e[5] & 2 and ambiguous(t) for e, t in zip(events, texts)) and any(not e[5] & 2 and ambiguous(t) for e, t in zip(events, texts))
    assert any(set(row[2]) == {"-"} and ambiguous(row[3]) for row in m.mutations())
    m.close(); db.close()


# ---------------------------------------------------------------- 4. the edge shapes of the stages, through the test entry

def device_text(mate_offset, mate_length, codes, events, query_base=0, cap=None):
    """xm_test_pileup_text -> (off, text, kernel launches)."""
    L = _capi.lib()
    events = np.ascontiguousarray(events, np.int64).reshape(-1, 8)
    mo, ml, cd = np.ascontiguousarray(mate_offset, np.int64), np.ascontiguousarray(mate_length, np.int32), np.ascontiguousarray(codes, np.uint8)
    n = len(events)
    want_bytes = int(tc.rule_text(mo, ml, cd, events, query_base)[0][-1]) if cap is None else cap
    off = np.full(n + 2, -7, np.int64)
    text = np.full(want_bytes + 8, 0x7E, np.uint8)
    launches = C.c_int32(-1)
    job = _capi.XmTestPileupJob(len(ml) // 2, mo.ctypes.data, ml.ctypes.data, cd.ctypes.data, len(cd), n, events.ctypes.data, query_base)
    if L.xm_test_pileup_text(0, C.byref(job), off.ctypes.data, text.ctypes.data, want_bytes, C.byref(launches)):
        raise RuntimeError(L.xm_last_error().decode())
    assert off[n + 1] == -7 and np.all(text[off[n]:] == 0x7E)
    return off[:n + 1].copy(), text[:off[n]].tobytes(), launches.value


MATES = tc.synthetic_mates(50, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 256 * 256 + 1])
def test_event_counts_on_the_scan_edges(n):
    """The scan's thread (16), gather-block (256) and block (4096) edges and 16 blocks plus one event: deletions interleaved with insertions of 1 .. 1000
    bases (a few bases each at the largest count), clipped events among them, a query base above 0."""
    lengths = (1, 1, 2, 3, 5, 63, 64, 65, 1000) if n <= 5000 else (1, 1, 1, 2, 2, 3, 5, 8, 64)
    events = tc.random_events(n, MATES[1], seed=100 + n, query_base=7_000_000_000, insert_lengths=lengths)
    want_off, want = tc.rule_text(*MATES, events, 7_000_000_000)
    off, text, launches = device_text(*MATES, events, 7_000_000_000)
    assert np.array_equal(off, want_off) and text == want
    assert launches == (0 if n == 0 else 5 if len(want) else 4)
    if n >= 255:
        assert len(want) > n // 2 and (events[:, 2] == 2).sum() > n // 5 and (np.diff(want_off)[events[:, 2] == 1] == 0).any()


@pytest.mark.gpu
def test_deletions_only_gather_nothing():
    events = tc.random_events(300, MATES[1], seed=21, deletions=1.0)
    off, text, launches = device_text(*MATES, events)
    assert not off.any() and text == b"" and launches == 4


@pytest.mark.gpu
def test_insertion_lengths_and_clipped_events():
    """Lengths 1, 63, 64, 65 and 1 000 at startA 0, in the middle and at readLen - length, both orientations, with deletions between them; then the events
    that keep less than their length or nothing."""
    mate_offset, mate_length, codes = MATES
    long_mate = int(np.nonzero(mate_length == 1200)[0][0])
    q, mate = long_mate // 2, long_mate & 1
    events = []
    for length in (1, 63, 64, 65, 1000):
        for start in (0, 100, 1200 - length):
            for rev in (0, 1):
                events.append(tc.event(q, mate, rev, start, length))
                events.append(tc.event(q, mate, rev, start, 4, kind=2))
    events += [tc.event(q, mate, 0, 1199, 5), tc.event(q, mate, 1, 1199, 5), tc.event(q, mate, 0, 1200, 5), tc.event(q, mate, 1, 5000, 5), tc.event(q, mate, 0, 3, 0),
               tc.event(q, mate, 0, -1, 5), tc.event(q, mate, 1, 200, 2**40), tc.event(50, 0, 0, 0, 5), tc.event(-1, 0, 0, 0, 5), tc.event(q, mate, 0, 600, -3)]
    want_off, want = tc.rule_text(mate_offset, mate_length, codes, events)
    assert list(np.diff(want_off)[-10:]) == [1, 1, 0, 0, 0, 0, 1000, 0, 0, 0] and set(np.diff(want_off)[:60:2]) == {1, 63, 64, 65, 1000}
    off, text, launches = device_text(mate_offset, mate_length, codes, events)
    assert np.array_equal(off, want_off) and text == want and launches == 5


@pytest.mark.gpu
def test_the_test_entry_refuses_mates_outside_of_codes_and_a_text_that_does_not_fit():
    mate_offset, mate_length, codes = MATES
    events = tc.random_events(40, mate_length, seed=5)
    with pytest.raises(RuntimeError, match="mate outside of codes"):
        device_text(mate_offset, mate_length, codes[:-1], events)
    with pytest.raises(RuntimeError, match="the text takes"):
        device_text(mate_offset, mate_length, codes, events, cap=3)


# ---------------------------------------------------------------- 5. the contract of the entries

@pytest.mark.gpu
def test_keep_insert_text_is_opt_in_set_before_the_first_add_and_changes_no_event():
    contigs, b = single_end_workload()
    db = api.ReferenceDatabase(contigs)
    align(db, b)
    off_m, on_m = pileup.MatchDatabase(db, 0.1), pileup.MatchDatabase(db, 0.1, keep_insert_text=True)
    L, h_off, h_on = off_m._L, off_m._h[0], on_m._h[0]
    assert L.xm_pileup_keep_insert_text(h_off, 1) == 0 and L.xm_pileup_keep_insert_text(h_off, 0) == 0   # (before the first add: any number of times)
    assert off_m.add_last() == on_m.add_last()
    assert L.xm_pileup_keep_insert_text(h_off, 1) != 0 and b"already added" in L.xm_last_error()
    assert L.xm_pileup_keep_insert_text(h_on, 0) != 0 and b"already added" in L.xm_last_error()
    assert L.xm_pileup_keep_insert_text(None, 1) != 0
    buf_off, buf_text = np.zeros(8, np.int64), np.zeros(64, np.uint8)
    assert L.xm_pileup_event_text(h_off, 0, 1, buf_off.ctypes.data, buf_text.ctypes.data, 64) == -1    # text was not kept
    assert L.xm_pileup_event_text(None, 0, 1, buf_off.ctypes.data, buf_text.ctypes.data, 64) == -1
    assert not buf_off.any() and not buf_text.any()
    assert sorted(off_m._events()) == sorted(on_m._events())
    for c in range(len(contigs)):
        assert np.array_equal(off_m._sum(c)[0], on_m._sum(c)[0]) and np.array_equal(off_m._sum(c)[1], on_m._sum(c)[1]) and np.array_equal(off_m._middle(c), on_m._middle(c))
    plain = [r for r in off_m.mutations() if set(r[2]) == {"-"}]
    assert plain and all(set(r[3]) == {"N"} for r in plain)   # (no source of text: N times the length)
    off_m.close(); on_m.close(); db.close()


@pytest.mark.gpu
def test_event_text_paging_and_life_after_the_context():
    contigs, b = single_end_workload()
    mates = W.mates_of(b)
    db = api.ReferenceDatabase(contigs)
    align(db, b)
    m = pileup.MatchDatabase(db, keep_insert_text=True)
    n = m.add_last(None)
    db.close()                                          # the context goes first: the text is host memory
    L, h = m._L, m._h[0]
    events = [e[1:] for e in m._events()]
    want = [t or "" for t in tc.insertion_texts(events, lambda ordinal: mates[ordinal])]
    total = sum(len(t) for t in want)
    got, off, text = page_text(L, h, 0, n + 5, total)
    assert got == n and text.decode() == "".join(want) and list(np.diff(off)) == [len(t) for t in want]
    for cap in (total - 1, 64, 7, 3):                   # smaller than the whole text: fewer events a page, as many as fit, never none
        first, pages, parts = 0, 0, []
        while first < n:
            got, off, text = page_text(L, h, first, n - first, cap)
            assert got >= 1 and (first + got == n or off[-1] + len(want[first + got]) > cap)
            parts.append(text.decode())
            assert list(np.diff(off)) == [len(t) for t in want[first:first + got]]
            first += got
            pages += 1
        assert "".join(parts) == "".join(want) and pages >= 2
    longest = max(range(n), key=lambda k: len(want[k]))
    assert len(want[longest]) >= 2
    assert page_text(L, h, longest, 5, len(want[longest]) - 1)[0] == -1 and page_text(L, h, longest, 1, len(want[longest]))[0] == 1   # one event that does not fit
    deletion = next(k for k in range(n) if events[k][2] == 2)
    got, off, text = page_text(L, h, deletion, 1, 0)     # an event without text fits into no bytes
    assert got == 1 and list(off) == [0, 0] and text == b""
    assert page_text(L, h, n, 4, 64)[0] == 0 and page_text(L, h, n + 1, 4, 64)[0] == -1 and page_text(L, h, -1, 4, 64)[0] == -1 and page_text(L, h, 0, 0, 64)[0] == 0
    assert L.xm_pileup_event_text(h, 0, 4, None, None, 64) == -1
    m.close()


# ---------------------------------------------------------------- 6. the command line

def write_fastq(path, reads, prefix="r"):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@%s%d\n%s\n+\n%s\n" % (prefix, i, api.decode(r), "I" * len(r)))


def run_job(tmp, tag, queries, extra):
    paths = {k: str(tmp / ("%s.%s" % (tag, k))) for k in ("mut", "sam", "un")}
    out = io.StringIO()
    assert cli.run(["--reference", str(tmp / "ref.fasta")] + queries + ["--out-mutations", paths["mut"], "--snp-threshold", "0", "0", "--indel-threshold", "0", "0",
                   "--distinguish-query-ends", "0.1", "--out-sam", paths["sam"], "--out-unaligned", paths["un"], "--batch-size", "128"] + extra, out=out) == 0
    return {k: open(p).read() for k, p in paths.items()}, out.getvalue()


@pytest.fixture(scope="module")
def single_job(tmp_path_factory):
    """900 reads against an 80 000-base reference (a few of them junk, for the unaligned file), written once; the per-object run is the reference."""
    tmp = tmp_path_factory.mktemp("mutations_job")
    ref = synth.synthetic_reference(80_000, seed=71)
    reads = list(synth.synthetic_single_end(ref, 880, seed=72, indel_prob=0.3)[0])
    rng = np.random.default_rng(73)
    for k in range(20):
        reads.insert(int(rng.integers(0, len(reads))), W.CODES[rng.integers(0, 4, 150)])
    with open(tmp / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(ref) + "\n")
    write_fastq(tmp / "reads.fastq", reads)
    queries = ["--queries", str(tmp / "reads.fastq")]
    return tmp, queries, run_job(tmp, "object", queries, ["--per-object"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", [("plain", []), ("parse_on_gpu", ["--parse-on-gpu"]), ("two_contexts", ["--devices", "0,0"])])
def test_cli_out_mutations_streams_and_writes_what_the_per_object_path_writes(single_job, name, extra):
    tmp, queries, (want_files, want_stats) = single_job
    body = [l.split("\t") for l in want_files["mut"].split("\n") if l and not l.startswith("#") and not l.startswith("CHR")]
    inserted = [l[3] for l in body if set(l[2]) == {"-"}]
    assert len(inserted) > 50 and all(set(t) <= set("ACGT") for t in inserted)   # insertion lines whose query allele is letters
    assert want_files["un"].count("\n") >= 80 and want_files["sam"].count("\n") > 880 and "Alignment rate" in want_stats
    seen = {}
    real = cli.native_source
    cli.native_source = lambda *a, **k: seen.setdefault("native", True) and real(*a, **k)   # (the job takes the streaming path)
    try:
        files, stats = run_job(tmp, name, queries, extra)
    finally:
        cli.native_source = real
    assert seen == {"native": True}
    for k in ("mut", "sam", "un"):
        assert files[k] == want_files[k], k
    assert stats == want_stats


@pytest.mark.gpu
def test_cli_out_mutations_of_pairs_with_spacing(tmp_path):
    ref = synth.synthetic_reference(60_000, seed=75)
    m1, m2 = synth.synthetic_paired_end(ref, 300, seed=76, indel_prob=0.3)[:2]
    with open(tmp_path / "ref.fasta", "w") as f:
        f.write(">chrSyn\n" + api.decode(ref) + "\n")
    write_fastq(tmp_path / "r1.fastq", m1, "p")
    write_fastq(tmp_path / "r2.fastq", m2, "p")
    queries = ["--paired-queries", str(tmp_path / "r1.fastq"), str(tmp_path / "r2.fastq"), "--spacing", "100", "50"]
    want_files, want_stats = run_job(tmp_path, "object", queries, ["--per-object"])
    files, stats = run_job(tmp_path, "plain", queries, [])
    body = [l.split("\t") for l in files["mut"].split("\n") if l and not l.startswith("#") and not l.startswith("CHR")]
    assert any(set(l[2]) == {"-"} and set(l[3]) <= set("ACGT") for l in body) and any(set(l[3]) == {"-"} for l in body)
    assert files == want_files and stats == want_stats
