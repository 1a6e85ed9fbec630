"""The end of --out-mutations on the device (xm_pileup_absorb, xm_pileup_call_snps, xm_pileup_judge_indels) against the host path, which is the
definition: synthetic counts through xm_test_pileup_call against pileup.CountedMatchDatabase over the same counts - on the edges of the wavefront, of the
select kernels' block and of the scan's levels, with contig starts inside blocks and wavefronts -, real alignments called by both paths of one MatchDatabase,
two contexts whose pile-ups are absorbed, the command line with and without --call-mutations-on-gpu, and the contract of the entries.  Every comparison is
equality of row lists or of file bytes."""
import ctypes as C
import io

import numpy as np
import pytest

import mutations_cases as mc
import oracle_lib
import pileup_workloads as W
from mapper_amd import _capi, api, cli, multi, pileup, synth

UNIT = mc.UNIT
FILTERS = mc.filters()


def block():
    return int(_capi.lib().xm_mutations_block_positions())


def c_filter(f):
    return _capi.XmMutationFilter(f.minSNPTotalDepth, f.minIndelTotalStartDepth, f.minIndelContinuationTotalDepth, f.minSNPDepthFraction, f.minIndelStartDepthFraction,
                                  f.minIndelContinuationDepthFraction, 0)


def device_call(lengths, sets, f, indels=(), with_middle=True, read_back=False):
    """xm_test_pileup_call over one or two sets of flat counts (depth, alt, middle) -> (xm_snp_row records, xm_indel_verdict records, the sets read back)."""
    L = _capi.lib()
    total = int(sum(lengths))
    lens = np.ascontiguousarray(lengths, np.int32)
    keep = [[np.ascontiguousarray(a, np.uint64) for a in s] for s in sets]
    candidates = pileup.indel_candidates(list(indels))
    verdicts = np.zeros(len(candidates), _capi.INDEL_VERDICT)
    back = [np.full((6 if with_middle else 5, total), 7, np.uint64) for _ in sets] if read_back else []
    filt = c_filter(f)
    job = _capi.XmTestMutationsJob(len(lens), len(sets), lens.ctypes.data)
    for s, (d, a, m) in enumerate(keep):
        assert d.shape == (total,) and a.shape == (4, total) and m.shape == (total,)
        job.depth[s], job.alt[s], job.middle[s] = d.ctypes.data, a.ctypes.data, m.ctypes.data if with_middle else None
        if read_back:
            job.read_back[s] = back[s].ctypes.data
    job.filter = C.pointer(filt)
    job.num_candidates, job.candidates, job.verdicts = len(candidates), candidates.ctypes.data, verdicts.ctypes.data
    calls = C.POINTER(_capi.XmSnpCalls)()
    if L.xm_test_pileup_call(0, C.byref(job), C.byref(calls)):
        raise RuntimeError(L.xm_last_error().decode())
    try:
        got = calls.contents
        n = int(got.num_rows)
        assert got.positions == total and bool(got.rows) == (n > 0) and got.bytes_to_host == (8 if n == 0 else 16 + 32 * n)
        snps = np.frombuffer((_capi.XmSnpRow * n).from_address(C.addressof(got.rows.contents)), dtype=_capi.SNP_ROW).copy() if n else np.zeros(0, _capi.SNP_ROW)
    finally:
        L.xm_snp_calls_free(calls)
    return snps, verdicts, back


def compare(lengths, depth, alt, middle, f, events=(), fraction=0.1, sets=None):
    """The device's rows over the counts (or over `sets`, whose sum they are) equal the host's -> (rows, verdicts)."""
    fed = mc.counted(lengths, depth, alt, middle if fraction > 0 else depth, events, fraction)
    want = fed.mutations(f)
    indels = list(fed._indels().items())
    snps, verdicts, _ = device_call(lengths, sets or [(depth, alt, middle)], f, indels, with_middle=fraction > 0)
    assert not snps["reference_code"].any()
    got = mc.rows_from(fed, snps, indels, verdicts)
    assert got == want
    return want, verdicts


LAYOUTS = {"one_base": lambda B: [1], "wave_edges": lambda B: [63, 1, 64], "block_edges": lambda B: [B - 1, 2, B, 1]}


def density_counts(total, density, seed):
    if density == "none":
        depth, alt, middle = mc.random_counts(total, 0.0, seed)
    elif density == "full":
        depth, alt, middle = mc.random_counts(total, 1.0, seed)
        alt[:] = np.minimum(alt, depth[None, :])
    elif density == "sparse":
        depth, alt, middle = mc.random_counts(total, 0.03, seed)
    else:  # rows in the first and the last position only
        depth, alt, middle = mc.random_counts(total, 0.0, seed)
        alt[:, 0] = depth[0]
        alt[1:3, -1] = depth[-1]
    return depth, alt, middle


# ---------------------------------------------------------------- 1. synthetic counts
@pytest.mark.gpu
@pytest.mark.parametrize("total", ["1", "63", "64", "65", "B-1", "B", "B+1"])
def test_totals_on_the_wavefront_and_block_edges(total):
    B = block()
    n = eval(total, {"B": B})
    assert B % 256 == 0 and B >= 256
    kept = judged = 0
    for k, density in enumerate(("none", "full", "sparse", "ends")):
        depth, alt, middle = density_counts(n, density, seed=100 + 7 * n + k)
        events = mc.random_events([n], 30, seed=n + k, flagged=0.2)
        sizes = {}
        for name, f in FILTERS.items():
            rows, verdicts = compare([n], depth, alt, middle, f, events)
            sizes[name] = (sum(1 for r in rows if "-" not in r[2] + r[3]), int((verdicts["keep"] > 0).sum()), len(verdicts))
        if density == "none":
            assert all(s[0] == 0 for s in sizes.values())
        if density == "full":   # four rows a position: the offsets at their maximum
            assert sizes["empty"][0] == 4 * n
            if n >= 63:
                assert 0 < sizes["half"][0] < 4 * n   # kept and dropped rows both exist
        if density == "ends":
            assert sizes["empty"][0] == (4 if n == 1 else 6)
        assert sizes["empty"][1] == sizes["empty"][2] > 0
        kept, judged = kept + sizes["half"][1], judged + sizes["half"][2]
    assert 0 < kept < judged or n == 1   # candidates on both sides of the indel thresholds


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("density", ["none", "full", "sparse", "ends"])
def test_contig_starts_inside_wavefronts_and_blocks(layout, density):
    lengths = LAYOUTS[layout](block())
    total = sum(lengths)
    depth, alt, middle = density_counts(total, density, seed=31 + total)
    events = mc.random_events(lengths, 40, seed=total, flagged=0.2)
    for fraction in (0.0, 0.1):
        for name, f in FILTERS.items():
            rows, _ = compare(lengths, depth, alt, middle, f, events if fraction else [e for e in events if not e[5] & 4], fraction)
            if name == "empty" and density == "full":
                assert [(r[0], r[1]) for r in rows if "-" not in r[2] + r[3]] == [(c, p + 1) for c, n in enumerate(lengths) for p in range(n) for _ in range(4)]
                assert set(r[0] for r in rows if "-" in r[2] + r[3]) == set(range(len(lengths))) or layout == "one_base"


@pytest.mark.gpu
def test_a_total_that_needs_two_levels_of_the_block_scan_and_two_sets_absorbed():
    """More blocks than one block of the scan takes: the block counts are summed into a level above them and scanned back down.  The same counts dealt over
    two sets, the second absorbed into the first: the rows are those of the sums, the source reads back as zeros and the target as the sums (the alt planes
    are longer than one pass of the absorb kernel's grid)."""
    B = block()
    total = B * 1024 + 5
    lengths = [total - 700_001, 700_000, 1]
    depth, alt, middle = mc.random_counts(total, 0.0005, seed=5)
    alt[:, 0] = depth[0]
    alt[:, -1] = depth[-1]
    alt[2, total - 700_001 - 1:total - 700_001 + 1] = UNIT   # the last base of contig 0 and the first of contig 1
    events = mc.random_events(lengths, 40, seed=6)
    rng = np.random.default_rng(8)
    first = [(a * rng.random(a.shape)).astype(np.uint64) for a in (depth, alt, middle)]
    second = [a - b for a, b in zip((depth, alt, middle), first)]
    fed = mc.counted(lengths, depth, alt, middle, events, 0.1)
    indels = list(fed._indels().items())
    for name in ("empty", "half"):
        f = FILTERS[name]
        want = fed.mutations(f)
        places = [r[:2] for r in want if "-" not in r[2] + r[3]]
        assert len(places) > 500 and (name != "empty" or (places[0] == (0, 1) and places[-1] == (2, 1) and (0, lengths[0]) in places and (1, 1) in places))
        snps, verdicts, _ = device_call(lengths, [(depth, alt, middle)], f, indels)
        assert mc.rows_from(fed, snps, indels, verdicts) == want
    snps, verdicts, back = device_call(lengths, [first, second], f, indels, read_back=True)
    assert mc.rows_from(fed, snps, indels, verdicts) == want
    assert not back[1].any()
    assert np.array_equal(back[0][0], depth) and np.array_equal(back[0][1:5], alt) and np.array_equal(back[0][5], middle)


@pytest.mark.gpu
@pytest.mark.parametrize("total,with_middle", [(1, True), (64, False), (257, True), (1030, False)])
def test_two_sets_absorbed_small(total, with_middle):
    lengths = [total] if total < 64 else [total - 40, 40]
    a, b = mc.random_counts(total, 0.3, seed=total), mc.random_counts(total, 0.3, seed=total + 1)
    summed = [x + y for x, y in zip(a, b)]
    fraction = 0.1 if with_middle else 0.0
    fed = mc.counted(lengths, summed[0], summed[1], summed[2] if with_middle else summed[0], (), fraction)
    for f in FILTERS.values():
        snps, _, back = device_call(lengths, [a, b], f, with_middle=with_middle, read_back=True)
        assert mc.rows_from(fed, snps, [], np.zeros(0, _capi.INDEL_VERDICT)) == fed.mutations(f)
        assert not back[1].any() and np.array_equal(back[0][0], summed[0]) and np.array_equal(back[0][1:5], summed[1])
        assert not with_middle or np.array_equal(back[0][5], summed[2])
    assert len(fed.mutations(FILTERS["empty"])) > len(fed.mutations(FILTERS["half"])) > 0 or total == 1


# ---------------------------------------------------------------- 2. real alignments: the host path against the device path of one MatchDatabase
REAL = mc.Filter(5.0, 0.08, 1.0, 0.08, 3.0, 0.08)   # (beside the empty and the default filter: one that keeps rows of a deep pile-up of sequencing errors and cuts deletions)


def align(db, b):
    return db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())


def shapes(rows):
    """-> (SNP rows, insertion rows, deletion rows)."""
    return (sum(1 for r in rows if "-" not in r[2] + r[3]), sum(1 for r in rows if set(r[2]) == {"-"}), sum(1 for r in rows if set(r[3]) == {"-"}))


def cut_deletions(everything, rows):
    """Deletion rows of `rows` that are shorter than the row of the same place and depth among `everything` (the empty filter's rows)."""
    whole = {}
    for c, pos1, ra, qa, w, _ in everything:
        if set(qa) == {"-"}:
            whole[(c, pos1, w)] = max(whole.get((c, pos1, w), 0), len(qa))
    return sum(1 for c, pos1, ra, qa, w, _ in rows if set(qa) == {"-"} and len(qa) < whole.get((c, pos1, w), 0))


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["overlapping_pairs", "three_batches", "several_contigs"])
def test_real_alignments_called_by_both_paths(workload):
    contigs, batches = getattr(W, workload)()
    db = api.ReferenceDatabase(contigs)
    ms = [pileup.MatchDatabase(db, fraction) for fraction in (0.0, 0.1)]
    for b in batches:
        align(db, b)
        mates = W.mates_of(b)
        for m in ms:
            m.add_last(mates)
    for m in ms:
        everything = m.mutations(mc.Filter.emptyFilter())
        snps, insertions, deletions = shapes(everything)
        assert snps > 50 and insertions > 10 and deletions > 10, (workload, snps, insertions, deletions)
        assert len(set(r[0] for r in everything)) == len(contigs)
        cut = 0
        for f in (mc.Filter.emptyFilter(), mc.Filter.defaultFilter(), REAL):
            host = m.mutations(f)
            device = m.mutations(f, on_gpu=True)
            assert device == host
            assert m.mutations(f) == host   # (the device path moved no count away)
            cut += cut_deletions(everything, host)
        if workload != "overlapping_pairs":   # (single reads at a depth of 30: deletions that continue under less than three reads of middle depth)
            assert cut > 0, workload
        assert m.last_on_gpu["bytes_to_host"] < 64 * (len(everything) + 1) and m.last_on_gpu["snp_rows"] <= snps
    for m in ms:
        m.close()
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0], [0, 1]], ids=["one_gpu", "two_gpus"])
def test_two_contexts_with_their_own_pileups_give_the_rows_of_one(devices):
    """Batches dealt between two contexts, each with its own pile-up: the device path absorbs the second into the first and gives the rows one context over
    all batches gives; the host path, which sums the replicas, gives them before and after."""
    if devices[1] >= _capi.lib().xm_device_count():
        pytest.skip("needs two GPUs (the peer copy of xm_pileup_absorb)")
    ref = synth.synthetic_reference(30_000, seed=61)
    contigs = [("a", ref[:18_000]), ("b", ref[18_000:])]
    reads = list(synth.synthetic_single_end(ref[:18_000], 1200, seed=62, indel_prob=0.4)[0]) + list(synth.synthetic_single_end(ref[18_000:], 800, seed=63, indel_prob=0.4)[0])
    order = np.random.default_rng(64).permutation(len(reads))
    batches = [oracle_lib.QueryBatch([W.single(reads[i]) for i in order[k::4]]) for k in range(4)]
    f = mc.Filter(3.0, 0.05, 1.0, 0.05, 1.0, 0.05)
    db = api.ReferenceDatabase(contigs)
    one = pileup.MatchDatabase(db, 0.1)
    for b in batches:
        align(db, b)
        one.add_last(W.mates_of(b))
    want = one.mutations(f)
    assert all(n > 20 for n in shapes(want)) and one.mutations(f, on_gpu=True) == want
    two = multi.MultiGpuDatabase(contigs, devices)
    m2 = pileup.MatchDatabase(two.replicas, 0.1)
    for k, b in enumerate(batches):
        align(two.replicas[k & 1], b)
        m2.add_last(W.mates_of(b), replica=k & 1)
    before = [m2._sum(c) for c in range(2)]
    assert m2.mutations(f) == want
    assert m2.mutations(f, on_gpu=True) == want
    # the counts moved: the second pile-up is empty, the first holds the sums, and the host path gives what it gave
    d = np.zeros(len(contigs[0][1]), np.uint64); a = np.zeros((4, len(d)), np.uint64)
    assert m2._L.xm_pileup_read(m2._h[1], 0, 0, len(d), d.ctypes.data, a.ctypes.data) == 0 and not d.any() and not a.any()
    assert m2._L.xm_pileup_read_middle(m2._h[1], 0, 0, len(d), d.ctypes.data) == 0 and not d.any()
    assert m2._L.xm_pileup_read(m2._h[0], 0, 0, len(d), d.ctypes.data, a.ctypes.data) == 0 and np.array_equal(d, before[0][0]) and np.array_equal(a, before[0][1])
    assert m2.mutations(f) == want and m2.mutations(f, on_gpu=True) == want
    assert m2.mutations(mc.Filter.emptyFilter(), on_gpu=True) == one.mutations(mc.Filter.emptyFilter())
    one.close(); m2.close(); db.close(); two.close()


# ---------------------------------------------------------------- 3. the command line
def run_job(tmp, tag, extra, sam=True):
    paths = {k: str(tmp / ("%s.%s" % (tag, k))) for k in ("mut", "sam")}
    out = io.StringIO()
    argv = ["--reference", str(tmp / "ref.fasta"), "--queries", str(tmp / "reads.fastq"), "--out-mutations", paths["mut"], "--snp-threshold", "2", "0.05", "--indel-threshold", "1", "0.05",
            "--batch-size", "128"] + (["--out-sam", paths["sam"]] if sam else []) + extra
    assert cli.run(argv, out=out) == 0
    return {k: open(p, "rb").read() for k, p in paths.items() if sam or k == "mut"}, out.getvalue()


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("call_mutations_job")
    ref = synth.synthetic_reference(40_000, seed=71)
    reads = list(synth.synthetic_single_end(ref[:25_000], 600, seed=72, indel_prob=0.4)[0]) + list(synth.synthetic_single_end(ref[25_000:], 300, seed=73, indel_prob=0.4)[0])
    with open(tmp / "ref.fasta", "w") as f:
        f.write(">chrA\n" + api.decode(ref[:25_000]) + "\n>chrB\n" + api.decode(ref[25_000:]) + "\n")
    with open(tmp / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
    return tmp, run_job(tmp, "host", [])


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", [("plain", []), ("two_contexts", ["--contexts", "2"]), ("two_contexts_parse", ["--contexts", "2", "--parse-on-gpu"]),
                                        ("on_gpu", ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"]),
                                        ("on_gpu_two_contexts", ["--contexts", "2", "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"])])
def test_cli_writes_the_same_files_with_the_flag(job, name, extra):
    tmp, (want_files, want_stats) = job
    body = [l.split(b"\t") for l in want_files["mut"].split(b"\n") if l and not l.startswith(b"#") and not l.startswith(b"CHR")]
    assert len(body) > 100 and {l[0] for l in body} == {b"chrA", b"chrB"} and any(set(l[2]) == {ord("-")} for l in body) and any(set(l[3]) == {ord("-")} for l in body)
    assert want_files["sam"].count(b"\n") > 900 and "Alignment rate" in want_stats
    files, stats = run_job(tmp, name, extra + ["--call-mutations-on-gpu"])
    assert files["mut"] == want_files["mut"] and files["sam"] == want_files["sam"] and stats == want_stats
    if extra and "--format-on-gpu" not in extra:   # (without the flag the device formatter still excludes --out-mutations)
        files, stats = run_job(tmp, name + "_host", extra)
        assert files == want_files and stats == want_stats


# ---------------------------------------------------------------- 4. the contract of the entries
def small_pileups():
    ref = synth.synthetic_reference(6_000, seed=5)
    contigs = [("long", ref), ("short", synth.synthetic_reference(2_000, seed=6))]
    return contigs, oracle_lib.QueryBatch(W.noisy_reads(ref, 64, 7))


@pytest.mark.gpu
def test_absorb_refuses_what_it_cannot_add():
    contigs, b = small_pileups()
    db, other = api.ReferenceDatabase(contigs), api.ReferenceDatabase(contigs[:1])
    m, n, with_ends, elsewhere = pileup.MatchDatabase(db), pileup.MatchDatabase(db), pileup.MatchDatabase(db, 0.1), pileup.MatchDatabase(other)
    L = m._L
    align(db, b)
    m.add_last(); n.add_last(); with_ends.add_last()
    depth = m._sum(0)[0]
    for into, source, message in ((None, m._h[0], b"null argument"), (m._h[0], None, b"null argument"), (m._h[0], m._h[0], b"the same pile-up was given twice"),
                                  (m._h[0], elsewhere._h[0], b"different indexes"), (m._h[0], with_ends._h[0], b"different query-end fractions"),
                                  (with_ends._h[0], m._h[0], b"different query-end fractions")):
        assert L.xm_pileup_absorb(into, source) != 0 and message in L.xm_last_error(), message
    assert np.array_equal(m._sum(0)[0], depth) and np.array_equal(n._sum(0)[0], depth)   # a refused call moved nothing
    assert L.xm_pileup_absorb(m._h[0], n._h[0]) == 0
    assert np.array_equal(m._sum(0)[0], 2 * depth) and not n._sum(0)[0].any() and not n._sum(0)[1].any() and depth.any()
    assert L.xm_pileup_absorb(m._h[0], n._h[0]) == 0 and np.array_equal(m._sum(0)[0], 2 * depth)   # (an empty pile-up adds nothing)
    assert len(n._events()) == len(m._events()) > 0   # the events stay with the pile-up that collected them
    for x in (m, n, with_ends, elsewhere):
        x.close()
    db.close(); other.close()


@pytest.mark.gpu
def test_calls_without_rows_or_candidates_leave_nothing_behind_and_need_no_context():
    contigs, b = small_pileups()
    db = api.ReferenceDatabase(contigs)
    m = pileup.MatchDatabase(db, 0.1)
    L, h = m._L, m._h[0]
    filt = c_filter(mc.Filter.emptyFilter())
    calls = C.POINTER(_capi.XmSnpCalls)()
    for p, f, out in ((None, C.byref(filt), C.byref(calls)), (h, None, C.byref(calls)), (h, C.byref(filt), None)):
        assert L.xm_pileup_call_snps(p, f, out) != 0 and b"null argument" in L.xm_last_error()
    L.xm_snp_calls_free(None)
    # an empty pile-up: no rows, no buffer, and nothing pinned that was not pinned before
    pinned = _capi.pinned_host_bytes()[0]
    assert L.xm_pileup_call_snps(h, C.byref(filt), C.byref(calls)) == 0
    assert calls.contents.num_rows == 0 and not calls.contents.rows and calls.contents.positions == 8_000 and calls.contents.bytes_to_host == 8
    L.xm_snp_calls_free(calls)
    assert m.mutations(on_gpu=True) == [] == m.mutations()
    assert _capi.pinned_host_bytes()[0] == pinned
    # no candidates: nothing to launch, whatever the arrays are
    assert L.xm_pileup_judge_indels(h, C.byref(filt), None, 0, None) == 0
    assert L.xm_pileup_judge_indels(h, C.byref(filt), None, -1, None) != 0 and b"negative size" in L.xm_last_error()
    one = pileup.indel_candidates([((0, 5, 2, "ACG", "---"), UNIT)])
    verdict = np.zeros(1, _capi.INDEL_VERDICT)
    for p, f, cand, out in ((None, C.byref(filt), one.ctypes.data, verdict.ctypes.data), (h, None, one.ctypes.data, verdict.ctypes.data), (h, C.byref(filt), None, verdict.ctypes.data),
                            (h, C.byref(filt), one.ctypes.data, None)):
        assert L.xm_pileup_judge_indels(p, f, cand, 1, out) != 0 and b"null argument" in L.xm_last_error()
    for field, value, message in (("contig", 2, b"contig outside of the reference"), ("contig", -1, b"contig outside of the reference"), ("kind", 0, b"kind must be 1"), ("kind", 3, b"kind must be 1")):
        bad = one.copy()
        bad[field] = value
        assert L.xm_pileup_judge_indels(h, C.byref(filt), bad.ctypes.data, 1, verdict.ctypes.data) != 0 and message in L.xm_last_error()
    assert L.xm_pileup_judge_indels(h, C.byref(filt), one.ctypes.data, 1, verdict.ctypes.data) == 0 and tuple(verdict[0]) == (0, 3)   # (no depth, no thresholds: kept whole)
    # with rows: the buffer comes from the pool and goes back to it; the pile-up outlives its context
    align(db, b)
    m.add_last(W.mates_of(b))
    want = m.mutations()
    db.close()
    assert len(want) > 20 and m.mutations(on_gpu=True) == want
    held = _capi.pinned_host_bytes()[0]
    assert m.mutations(on_gpu=True) == want and _capi.pinned_host_bytes()[0] == held
    m.close()
