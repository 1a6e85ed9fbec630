"""GPU tier: the queries of a batch counted per combination of contigs on the GPU (xm_refs_count_last, api.ReferenceDatabase.refs_count_last,
`--count-refs-on-gpu`; the kernels of mapper_amd/csrc/xm_refs.h over the rules of xm_refs_rules.h).  The yardstick is refs_cases.recount - cli.ObjectSink's
expression over decoded slices -, which tests/test_refs_rules.py holds equal to the C++ rules on the CPU.  Every comparison is of whole dicts, after the host's
fold of the left-over queries: at the edges of the wavefront, the block and the scan block; one hot combination; every query its own; sets of 8, 9 and 40
contigs; fingerprints of three bits, which collide, for the same dict; whole fingerprints, which must leave the host nothing; a malformed slice fails the call
with the query named and the next call works.  On real alignments the count is the one made of query_alignments on the host, with and without the copy of the
streams, it is refused once the batch is gone, and the command line writes the same file with and without the flag."""
import ctypes as C
import io
import os

import pytest

import refs_cases as rc
import sam_cases as sc
import summary_cases as sm
from mapper_amd import _capi, api, cli, synth

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4200]


def gpu_count(arrays, num_contigs=rc.NUM_CONTIGS, bits=64):
    """xm_test_refs_count on four streams -> an api.RefsCount; RuntimeError with the library's message."""
    L = _capi.lib()
    ints, dbls, io_, do = arrays
    out = C.POINTER(_capi.XmRefsCount)()
    if L.xm_test_refs_count(0, len(io_) - 1, num_contigs, ints.ctypes.data, dbls.ctypes.data, io_.ctypes.data, do.ctypes.data, bits, C.byref(out)):
        assert not out
        raise RuntimeError(L.xm_last_error().decode())
    return api.RefsCount(L, out)


def check(streams, num_contigs=rc.NUM_CONTIGS, bits=64, leftover=None, what=""):
    arrays = sm.arrays_of(streams)
    want = rc.recount(arrays, num_contigs)
    got = gpu_count(arrays, num_contigs, bits)
    assert got.counts() == want, what
    assert got.num_queries == len(arrays[2]) - 1 and got.num_aligned == sum(want.values())
    assert sum(c for _, c in got.records) + got.num_leftover_queries == got.num_aligned and len({ids for ids, _ in got.records}) == got.num_combinations
    assert all(1 <= len(ids) <= 8 and list(ids) == sorted(set(ids)) and c >= 1 for ids, c in got.records)
    assert (got.kernel_ms > 0 and got.d2h_ms >= 0) if got.num_queries else got.kernel_ms == 0
    if leftover is not None:
        assert got.num_leftover_queries == leftover, what   # (a condition: the device, not the host's fold, did the counting)
    return want, got


@pytest.mark.parametrize("nq", EDGES)
def test_query_counts_at_the_wave_block_and_scan_edges(nq):
    streams = rc.random_streams(nq)
    want, _ = check(streams, leftover=0, what=nq)
    assert sum(want.values()) >= 0.6 * nq and (nq < 63 or len(want) >= 8)
    if nq >= 63:
        _, got = check(streams, bits=3, what=(nq, "three bits"))
        assert got.num_leftover_queries > 0


def test_every_aligned_query_on_the_same_combination():
    want, got = check(rc.same_combination_case(4200), leftover=0)
    assert want == {(1, 3): 3360} and got.records == [((1, 3), 3360)]


def test_no_query_is_aligned():
    want, got = check(sc.all_unaligned_case(300)[1], leftover=0)
    assert want == {} and got.num_combinations == 0 and got.num_aligned == 0


def test_every_query_its_own_combination():
    own = rc.own_combination_case(4097, 300)
    want, got = check(own, num_contigs=300, leftover=0)
    assert len(want) == 4097 and got.num_combinations == 4097
    _, got = check(own, num_contigs=300, bits=3)
    assert got.num_leftover_queries >= 4090


def test_sets_of_eight_nine_and_forty_contigs():
    want, got = check(rc.set_sizes_case(), num_contigs=40, leftover=3)
    assert want == {(0,): 2, tuple(range(10, 18)): 3, tuple(range(9)): 2, tuple(range(40)): 1}
    assert sorted(got.records) == [((0,), 2), (tuple(range(10, 18)), 3)]
    lo = got.leftover_offsets
    assert [int(lo[k + 1] - lo[k]) for k in range(3)] == [9, 40, 9] and list(got.leftover_contigs[:9]) == list(range(9))   # (stream order)


def test_a_repeated_contig_a_pair_and_a_fallen_back_pair():
    want, _ = check(rc.shapes_case(), leftover=0)
    assert want == {(2,): 1, (0, 1): 1, (0, 3): 1, (3,): 1}
    check(sc.shapes_case()[1], leftover=0)


@pytest.mark.parametrize("nq,at", [(65, 63), (300, 256), (4200, 4096)])
def test_a_wide_query_between_unaligned_ones(nq, at):
    want, got = check(rc.wide_between_unaligned_case(nq, at), num_contigs=64, leftover=1)
    assert want == {tuple(range(40)): 1} and got.num_combinations == 0 and list(got.leftover_contigs) == list(range(40))


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # formatRange accepts them when it writes no SAM (tests/test_summary_rules.py)


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_every_malformed_condition_fails_the_call_and_the_next_call_works(name):
    arrays = sc.malformed_cases()[name][1].arrays()
    lowest = 4 if name in SAM_ONLY else 2   # (query 4 is malformed in every case; query 2 only where the summary rejects it without a SAM file)
    with pytest.raises(RuntimeError, match="malformed result streams: query %d$" % lowest):
        gpu_count(arrays)
    four = sm.first_queries(arrays, 4)
    if name in SAM_ONLY:
        check(four)
    else:
        with pytest.raises(RuntimeError, match="malformed result streams: query 2$"):
            gpu_count(four)
    check(rc.random_streams(300, seed=5), what="after the error")


# ---------------------------------------------------------------- real alignments
@pytest.fixture(scope="module")
def two_contigs(tmp_path_factory):
    """Two contigs with reads from each (tests/test_gpu_pileup.py::test_cli_out_refs_map_count's job), and twenty reads from neither."""
    d = tmp_path_factory.mktemp("refs_count")
    a, b = synth.synthetic_reference(60_000, seed=81), synth.synthetic_reference(40_000, seed=82)
    elsewhere = synth.synthetic_reference(5_000, seed=85)
    reads = list(synth.synthetic_single_end(a, 300, seed=83)[0]) + list(synth.synthetic_single_end(b, 200, seed=84)[0]) + list(synth.synthetic_single_end(elsewhere, 20, seed=86)[0])
    with open(d / "ref.fasta", "w") as f:
        f.write(">chrA\n" + api.decode(a) + "\n>chrB\n" + api.decode(b) + "\n")
    with open(d / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
    contigs = api.sort_reference([("chrA", api.decode(a)), ("chrB", api.decode(b))])
    return dict(ref=str(d / "ref.fasta"), reads=str(d / "reads.fastq"), contigs=contigs, queries=[api.Query(api.decode(r), name="r%d" % i) for i, r in enumerate(reads)])


def host_count(result):
    out = {}
    for q in range(len(result)):
        comps = result.query_alignments(q)
        if any(len(c) > 0 for c in comps):
            key = tuple(sorted({sa.contig for comp in comps for al in comp for sa in al.components}))
            out[key] = out.get(key, 0) + 1
    return out


def test_the_count_of_real_alignments_with_and_without_the_copy_and_its_residency(two_contigs):
    db = api.ReferenceDatabase(two_contigs["contigs"], mode="mapper", max_query_length=200)
    try:
        arrays = api.ReferenceDatabase.batch_arrays(two_contigs["queries"])
        db.upload_arrays(*arrays)
        first = db.align_resident(PARAMS)
        want = host_count(first)
        assert set(want) >= {(0,), (1,)} and want[(0,)] >= 195 and want[(1,)] >= 195 and 490 <= sum(want.values()) <= 520
        assert db.refs_count_last() == want
        raw = db.refs_count_last(raw=True)
        assert raw.num_queries == 520 and raw.num_aligned == sum(want.values()) and raw.num_leftover_queries == 0 and raw.kernel_ms > 0
        db.set_result_copy(False)
        second = db.align_resident(PARAMS)
        assert second.int_off is None and db.refs_count_last() == want
        summary = db.summary_last()
        assert summary.num_aligned == raw.num_aligned   # (beside the summary, on the same resident streams)
        summary.close()
        # the next batch is staged and committed: the count is refused, and serves again after the next align call
        db.stage_arrays(*api.ReferenceDatabase.batch_arrays(two_contigs["queries"][:100]))
        db.commit_staged()
        with pytest.raises(RuntimeError, match="the batch of the last align call is no longer resident"):
            db.refs_count_last()
        db.align_resident(PARAMS)
        assert sum(db.refs_count_last().values()) >= 95
    finally:
        db.close()


def run_job(argv, out_dir, outputs):
    os.makedirs(out_dir)
    log = io.StringIO()
    assert cli.run(argv + [x for flag, name in outputs for x in (flag, str(out_dir / name))], out=log) == 0
    text = log.getvalue()
    return tuple(open(out_dir / name, "rb").read() for _, name in outputs) + (text[text.index("Statistics"):],)


@pytest.mark.parametrize("name,flags,sam", [
    ("alone", [], False),
    ("everything_on_the_gpu", ["--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"], True),
    ("small_batches", ["--batch-size", "128"], False),
    ("two_contexts", ["--batch-size", "128", "--contexts", "2"], False),
])
def test_command_line_writes_the_same_counts_with_the_flag(two_contigs, tmp_path, name, flags, sam):
    base = ["--reference", two_contigs["ref"], "--queries", two_contigs["reads"]]
    outputs = (("--out-refs-map-count", "counts.txt"),) + ((("--out-sam", "out.sam"),) if sam else ())
    # (without the flag --out-refs-map-count excludes the other three: the per-object job runs with the batch size and the contexts only)
    plain = run_job(base + [f for f in flags if not f.endswith("-on-gpu")], tmp_path / "plain", outputs)
    counts = dict(line.split("\t") for line in plain[0].decode().split("\n") if line)
    assert int(counts["chrA"]) >= 295 and int(counts["chrB"]) >= 195 and sum(int(v) for v in counts.values()) <= 520
    got = run_job(base + flags + ["--count-refs-on-gpu"], tmp_path / "flag", outputs)
    assert got == plain, name
    if sam:
        assert len(got[1]) > 50_000 and got[1].startswith(b"@HD")
