"""GPU tier: the results left in HBM (xm_context_set_result_copy, xm_summary_last, api.ReferenceDatabase.set_result_copy / summary_last, `--results-on-gpu`;
the kernels of mapper_amd/csrc/xm_summary.h over the rules of xm_summary_rules.h).  The yardstick for the summary is summary_cases.recount, a count written
in Python from the stream layout, which tests/test_summary_rules.py holds equal to the C++ rules on the CPU: counts, list and penalties (bit for bit) at the
edges of the wavefront, the gather block and the scan block; a malformed slice fails the call with the query named and the next call works.  On real
alignments an align call without the copy leaves a result without streams and everything made of the resident streams - summary, SAM text, the writer's
files and statistics - is what is made of the copied ones; the summary is refused once the batch is gone or the call failed; the command line writes the
same bytes with and without the flag."""
import ctypes as C
import io
import os
import struct
import tempfile

import numpy as np
import pytest

import oracle_lib as o
import pair_geometry as pg
import pileup_workloads as pw
import sam_cases as sc
import summary_cases as sm
from mapper_amd import _capi, api, cli, hostio, synth
from test_gpu_sam import JOBS, fastq_of, letters, work  # noqa: F401  (the fixture with the 2 100 singles and the pairs as FASTQ files, and the two jobs over them)

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()


def gpu_summary(arrays, want_unaligned=True, num_contigs=sm.NUM_CONTIGS, nq=None):
    """xm_test_summary on four streams -> an api.BatchSummary; RuntimeError with the library's message."""
    L = _capi.lib()
    ints, dbls, io_, do = arrays
    nq = len(io_) - 1 if nq is None else nq
    out = C.POINTER(_capi.XmBatchSummary)()
    if L.xm_test_summary(0, nq, num_contigs, ints.ctypes.data, dbls.ctypes.data, io_.ctypes.data, do.ctypes.data, 1 if want_unaligned else 0, C.byref(out)):
        assert not out
        raise RuntimeError(L.xm_last_error().decode())
    return api.BatchSummary(L, out)


def check(streams, what=""):
    arrays = sm.arrays_of(streams)
    want = sm.recount(arrays)
    for want_unaligned in (True, False):
        got = gpu_summary(arrays, want_unaligned)
        assert sm.same(got, want, want_unaligned), what
        assert got.kernel_ms > 0 and got.d2h_ms >= 0
        got.close()
    return want


# ---------------------------------------------------------------- summaries of given streams
def test_every_shape():
    want = check(sc.shapes_case()[1], "shapes")
    assert want.num_queries == 25 and list(want.unaligned) == [2, 10, 16] and max(want.alignments) == 4


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4200])
def test_query_counts_at_the_wave_block_and_scan_edges(nq):
    want = check(sc.random_case(100 + nq, nq, read_len=None if nq < 1000 else 24, name_len=5, unaligned=0.2 if nq > 1 else 0.0)[1], nq)
    assert want.num_queries == nq and want.num_alignments >= want.num_aligned and (nq < 63 or (want.num_aligned >= 0.6 * nq and want.num_unaligned > 0))


@pytest.mark.parametrize("unaligned", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_streams(seed, unaligned):
    check(sc.random_case(seed, 400, unaligned=unaligned)[1], (seed, unaligned))


def test_no_query_at_all_launches_nothing_and_gives_zeros():
    empty = (np.zeros(1, np.int32), np.zeros(1, np.float64), np.zeros(1, np.int64), np.zeros(1, np.int64))
    got = gpu_summary(empty, nq=0)
    assert (got.num_queries, got.num_aligned, got.num_alignments, got.total_aligned_length, got.num_indels, got.num_unaligned) == (0,) * 6
    assert len(got.penalties) == 0 and len(got.unaligned) == 0 and got.kernel_ms == 0
    got.close()


@pytest.mark.parametrize("nq", [64, 257, 4097])
def test_all_unaligned_and_none_unaligned(nq):
    want = check(sc.all_unaligned_case(nq)[1], "all unaligned")
    assert want.num_unaligned == nq and want.num_alignments == 0
    want = check(sm.none_unaligned_case(nq), "none unaligned")
    assert want.num_unaligned == 0 and want.num_alignments == nq


@pytest.mark.parametrize("nq,at", [(65, 63), (300, 256), (4200, 4096)])
def test_one_query_with_forty_alignments_between_queries_with_none(nq, at):
    want = check(sm.many_alignments_case(nq, at), (nq, at))
    assert want.alignments[at] == 40 and want.num_alignments == 40 and want.num_unaligned == nq - 1 and len(set(want.penalties.tolist())) == 40


def test_three_alignments_and_one_pair():
    assert check(sc.three_alignments_case()[1]).alignments == [3]
    assert check(sc.one_pair_case()[1]).num_indels == 2


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # formatRange accepts them when it writes no SAM (tests/test_summary_rules.py)


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_every_malformed_condition_fails_the_call_and_the_next_call_works(name):
    _, streams, _ = sc.malformed_cases()[name]
    arrays = streams.arrays()
    lowest = 4 if name in SAM_ONLY else 2   # (query 4 is malformed in every case; query 2 only where the host rejects it without a SAM file)
    with pytest.raises(sm.Malformed) as e:
        sm.recount(arrays)
    assert e.value.query == lowest
    with pytest.raises(RuntimeError, match="malformed result streams: query %d$" % lowest):
        gpu_summary(arrays)
    four = sm.first_queries(arrays, 4)
    if name in SAM_ONLY:
        check(four, "the first four queries")
    else:
        with pytest.raises(RuntimeError, match="malformed result streams: query 2$"):
            gpu_summary(four)
    check(sc.random_case(5, 300)[1], "after the error")


def test_a_malformed_slice_in_a_large_batch_names_the_lowest_query():
    ints, dbls, io_, do = sc.random_case(77, 4200, read_len=24, name_len=5, unaligned=0.0)[1].arrays()
    q = next(k for k in range(2000, 4200) if io_[k + 1] - io_[k] >= 11)
    later = next(k for k in range(4097, 4200) if io_[k + 1] - io_[k] >= 11 and k > q)
    bad = ints.copy()
    bad[io_[q]:io_[q] + 4] = [1, 1, 17, 3]
    bad[io_[later]:io_[later] + 4] = [1, 1, 17, 0]
    with pytest.raises(RuntimeError, match="malformed result streams: query %d$" % q):
        gpu_summary((bad, dbls, io_, do))
    check((ints, dbls, io_, do), "after the error")


# ---------------------------------------------------------------- real alignments
def names_of(mates):
    return [tuple(b"q%d/%d" % (q, k + 1) for k in range(len(m))) for q, m in enumerate(mates)]


def workload(name):
    """-> (contigs, the batch as a sam_cases.Batch with names, expected inner distances, deviations)."""
    if name == "singles":  # the 2 100 single reads of tests/test_gpu_sam.py's fixture
        contigs, _ = pw.fallback_pairs()
        elsewhere = synth.synthetic_reference(5_000, seed=98)
        reads = list(synth.synthetic_single_end(contigs[0][1], 2000, seed=51, indel_prob=0.3)[0]) + list(synth.synthetic_single_end(elsewhere, 100, seed=52)[0])
        mates = [(r,) for r in reads]
        return contigs, sc.Batch(mates, names_of(mates)), np.zeros(len(mates)), np.ones(len(mates))
    contigs, (qb,) = pw.fallback_pairs() if name == "fallback_pairs" else pw.many_equal_alignments()
    mates = [tuple(m) for m in pw.mates_of(qb)]
    return contigs, sc.Batch(mates, names_of(mates)), qb.expected_inner, qb.deviation


def kept_streams(r):
    return tuple(np.array(a) for a in (r.ints, r.dbls, r.int_off, r.dbl_off))


def written(names, batch, result, **kw):
    """What hostio.Writer makes of the batch -> (SAM bytes, the unaligned-query file, the five statistics bit for bit)."""
    with tempfile.TemporaryFile("w+b") as sam, tempfile.TemporaryFile("w+b") as un:
        w = hostio.Writer(names, sam, un, threads=2)
        w.write(batch, result, **kw)
        sam.seek(0); un.seek(0)
        st = w.stats
        return sam.read(), un.read(), (st.num_queries, st.num_aligned, st.total_aligned_length, st.num_indels, struct.pack("<d", st.total_penalty))


@pytest.mark.parametrize("name", ["fallback_pairs", "singles", "many_equal_alignments"])
def test_an_align_call_without_the_copy(name):
    contigs, batch, inner, deviation = workload(name)
    names = [n for n, _ in contigs]
    db = api.ReferenceDatabase(contigs)
    try:
        db.set_sam_contigs(names)
        db.upload_arrays(batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes[:max(batch.codes_length, 1)], inner, deviation)
        # 1. with the copy: the streams, and the shapes they hold
        first = db.align_resident(PARAMS)
        kept = kept_streams(first)
        want = sm.recount(kept, num_contigs=len(contigs))
        ints, io_ = kept[0], kept[2]
        fallback = sum(1 for q in range(len(batch)) if ints[io_[q]] == 2 and want.alignments[q] > 0)
        if name == "fallback_pairs":
            assert want.num_unaligned >= 15 and fallback > 30 and want.num_indels > 100
        elif name == "singles":
            assert len(batch) == 2100 and want.num_unaligned >= 90 and want.num_indels > 300
        else:
            assert {2, 23} <= set(want.alignments) and max(want.alignments) >= 23 and want.num_alignments > 2 * want.num_aligned
        want_files = written(names, batch, first)
        # 2. without it: no streams, the same totals and counters, and no pinned memory for streams (the first result still holds its own)
        pinned_before, _ = _capi.pinned_host_bytes()
        db.set_result_copy(False)
        second = db.align_resident(PARAMS)
        pinned_after, _ = _capi.pinned_host_bytes()
        assert second.ints is None and second.dbls is None and second.int_off is None and second.dbl_off is None
        assert len(second) == len(batch) and second.num_ints == len(kept[0]) and second.num_dbls == len(kept[1])
        assert list(second.counters[:11]) == list(first.counters[:11]) and second.d2h_ms > 0
        assert pinned_after == pinned_before and kept[0].nbytes + kept[1].nbytes > 100_000
        with pytest.raises(ValueError, match="set_result_copy"):
            second.query_alignments(0)
        # 3. the summary of the resident streams
        for want_unaligned in (False, True):
            summary = db.summary_last(want_unaligned=want_unaligned)
            assert sm.same(summary, want, want_unaligned) and summary.kernel_ms > 0
            if not want_unaligned:
                summary.close()
        # 4. the text of the resident streams
        text = db.format_sam_last(batch)
        assert bytes(text) == want_files[0] and len(want_files[0]) > 100_000
        # 5. the writer with text and summary, and a result without streams
        assert written(names, batch, second, sam_text=text, summary=summary) == want_files
        text.close(); summary.close()
        # 6. the copy again
        db.set_result_copy(True)
        third = db.align_resident(PARAMS)
        assert all(np.array_equal(a, b) for a, b in zip(kept_streams(third), kept))
        # (the launches of a context's first call may include a pass that grew a result arena: the calls behind it compare like with like)
        assert third.kernel_launches == second.kernel_launches and list(third.counters[:12]) == list(second.counters[:12])
        got = db.summary_last(want_unaligned=True)   # (it works whether or not the copy is on)
        assert sm.same(got, want)
        got.close()
    finally:
        db.close()


def query_batch(queries):
    b = o.QueryBatch(queries)
    return b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation


def test_the_summary_is_refused_once_the_batch_is_gone_or_the_call_failed():
    contigs, _ = pg.reference()
    ordinary = pg.ordinary_queries(300)
    contained = pg.one_of_each_kind()["contained"][0]   # a mate inside its partner: the reference would have thrown
    refused = "the batch of the last align call is no longer resident"
    db = api.ReferenceDatabase(contigs)
    try:
        db.set_result_copy(False)
        db.upload_arrays(*query_batch(ordinary))
        r = db.align_resident(PARAMS)
        assert r.int_off is None
        good = db.summary_last(want_unaligned=True)
        assert good.num_queries == 300 and good.num_aligned > 250
        # the next batch is committed
        db.stage_arrays(*query_batch(ordinary[:100]))
        db.commit_staged()
        with pytest.raises(RuntimeError, match=refused):
            db.summary_last()
        r = db.align_resident(PARAMS)
        s = db.summary_last()
        assert s.num_queries == 100 and s.num_aligned > 80
        s.close()
        # an align call that fails
        db.upload_arrays(*query_batch(pg.with_throwers(ordinary, [(120, contained)])))
        with pytest.raises(RuntimeError, match="Failed to align query 120: the reference implementation would have thrown here"):
            db.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match=refused):
            db.summary_last()
        # the next good call serves again
        db.upload_arrays(*query_batch(ordinary))
        db.align_resident(PARAMS)
        again = db.summary_last(want_unaligned=True)
        assert sm.same(again, good)
        again.close(); good.close()
    finally:
        db.close()


# ---------------------------------------------------------------- the command line
def run_job(argv, out_dir, outputs):
    os.makedirs(out_dir)
    log = io.StringIO()
    assert cli.run(argv + [x for flag, name in outputs for x in (flag, str(out_dir / name))], out=log) == 0
    text = log.getvalue()
    phases = cli.last_timing["phases"]
    assert sorted(phases) == ["align", "format", "read", "stage", "write"] and all(v >= 0 for v in phases.values()) and phases["align"] > 0
    return tuple(open(out_dir / name, "rb").read() for _, name in outputs) + (text[text.index("Statistics"):],)


@pytest.mark.parametrize("name", sorted(JOBS))
def test_command_line_writes_the_same_bytes_with_the_flag(work, tmp_path, name):  # noqa: F811
    base = ["--reference", work["files"]["ref"]] + JOBS[name](work["files"])
    outputs = (("--out-sam", "sam"), ("--out-unaligned", "unaligned"))
    first = run_job(base, tmp_path / "plain", outputs)
    assert len(first[0]) > 100_000 and first[0].startswith(b"@HD") and first[1].count(b"\n+\n") >= (90 if name != "pairs" else 2) and "Alignment rate" in first[2]
    for k, flags in enumerate((["--format-on-gpu", "--results-on-gpu"], ["--format-on-gpu", "--results-on-gpu", "--parse-on-gpu"],
                               ["--format-on-gpu", "--results-on-gpu", "--parse-on-gpu", "--contexts", "2"])):
        got = run_job(base + flags, tmp_path / ("flags%d" % k), outputs)
        assert cli.last_timing["phases"]["format"] > 0
        assert got == first, flags


def test_command_line_mutations_and_no_output(tmp_path):
    contigs, batches = pw.three_batches()
    reads = [m[0] for b in batches for m in pw.mates_of(b)]
    assert len(reads) == 741
    open(tmp_path / "ref.fa", "wb").write(b"".join(b">" + n.encode() + b"\n" + letters(c) + b"\n" for n, c in contigs))
    open(tmp_path / "se.fq", "wb").write(fastq_of(reads, "read%d"))
    base = ["--reference", str(tmp_path / "ref.fa"), "--queries", str(tmp_path / "se.fq"), "--batch-size", "300"]
    outputs = (("--out-mutations", "mutations"), ("--out-unaligned", "unaligned"))
    first = run_job(base, tmp_path / "plain", outputs)
    assert len(first[0]) > 0 and first[1].count(b"\n+\n") >= 40
    assert run_job(base + ["--results-on-gpu"], tmp_path / "flag", outputs) == first
    assert run_job(base + ["--no-output", "--results-on-gpu"], tmp_path / "none", ()) == first[2:]


@pytest.mark.parametrize("flags,message", [
    (["--no-output", "--results-on-gpu", "--per-object"], "--results-on-gpu and --per-object exclude each other"),
    (["--out-refs-map-count", "counts.txt", "--results-on-gpu"], "--results-on-gpu and --out-refs-map-count exclude each other"),
    (["--out-sam", "out.sam", "--results-on-gpu"], "--results-on-gpu with --out-sam needs --format-on-gpu"),
    (["--out-sam", "out.sam", "--format-on-gpu", "--results-on-gpu", "--out-mutations", "m.txt"], "--format-on-gpu and --out-mutations exclude each other"),
])
def test_usage_errors_exit_with_status_1_and_their_message(work, capsys, flags, message):  # noqa: F811
    assert cli.main(["--reference", work["files"]["ref"], "--queries", work["files"]["se"]] + flags) == 1
    assert "Error: " + message in capsys.readouterr().err
