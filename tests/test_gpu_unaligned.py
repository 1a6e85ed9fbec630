"""GPU tier: the unaligned-query file written on the GPU and the staged batch kept in HBM (xm_unaligned_format_last, xm_context_set_batch_copy,
api.ReferenceDatabase.unaligned_format_last / set_batch_copy, `--unaligned-on-gpu`, `--batch-on-gpu`; the kernels of mapper_amd/csrc/xm_unaligned.h over the
rules of xm_unaligned_rules.h).  The yardstick everywhere is the host path: the unaligned-query file and the statistics that hostio.Writer (xmio_write_batch)
makes of the same batch and the same streams.  Kernels over given arrays (xm_test_unaligned_format): query counts at the edges of the wavefront, the block
and the scan block, every query and no query unaligned, record ends on both sides of the tile's multiples, a mate of 30 000 bases, one unaligned query between
4 096 aligned ones, no query at all, malformed slices.  Real alignments on a small reference whose every fifth read is random (tests/test_unaligned_rules.py
holds on the CPU that exactly those are unaligned): a job whose batch and streams stay in HBM gives the bytes and statistics of the job that copies both and
writes on the host; the qualities belong to the batch they came with; the refusals; the command line with and without the two flags."""
import ctypes as C
import io
import os
import subprocess
import sys
import tempfile

import pytest

import pair_geometry as pg
import pileup_workloads as pw
import sam_cases as sc
import summary_cases as sm
import unaligned_cases as uc
from mapper_amd import _capi, api, cli, hostio

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_unaligned(batch, streams, nq=None):
    """xm_test_unaligned_format on a batch and its streams -> (text, mates written, kernel ms); RuntimeError with the library's message."""
    L = _capi.lib()
    ints, dbls, io_, do = streams.arrays() if isinstance(streams, sc.Streams) else streams
    with_qual = batch.has_qual is not None
    job = _capi.XmTestUnalignedJob(len(batch) if nq is None else nq, batch.mate_count.ctypes.data, batch.mate_offset.ctypes.data, batch.mate_length.ctypes.data, batch.codes.ctypes.data,
                                   batch.codes_length, C.addressof(batch._names), batch.name_off.ctypes.data, C.addressof(batch._quals) if with_qual else None,
                                   batch.qual_off.ctypes.data if with_qual else None, batch.has_qual.ctypes.data if with_qual else None, len(sc.CONTIGS), 0,
                                   ints.ctypes.data, dbls.ctypes.data, io_.ctypes.data, do.ctypes.data)
    out = C.POINTER(_capi.XmSamText)()
    if L.xm_test_unaligned_format(0, C.byref(job), C.byref(out)):
        assert not out
        raise RuntimeError(L.xm_last_error().decode())
    t = api.SamText(L, out)
    try:
        assert t.h2d_ms == 0 and t.d2h_ms >= 0
        return bytes(t), t.records, t.kernel_ms
    finally:
        t.close()


def check(batch, streams, what=""):
    want, _ = uc.expected(batch, streams)
    text, mates, kernel_ms = gpu_unaligned(batch, streams)
    assert text == want, what
    listed = sm.recount(streams.arrays() if isinstance(streams, sc.Streams) else streams).unaligned
    assert mates == sum(int(batch.mate_count[q]) for q in listed) and kernel_ms > 0, what
    return text, len(listed)


# ---------------------------------------------------------------- the kernels over given arrays
def test_every_shape():
    batch, streams = uc.shapes_case()
    text, unaligned = check(batch, streams, "shapes")
    assert unaligned == 15 and b"@sixteen_codes\n?ACMGRSVTWYHKDBN\n+\n" in text and b"@" + b"n" * 300 + b"\n" in text and b"\n>\n" in text
    at = text.index(b"@thirty_thousand\n") + len(b"@thirty_thousand\n")   # the mate of 30 000 bases with its qualities
    assert text[at + 30_000:at + 30_003] == b"\n+\n" and text[at + 60_003:at + 60_004] == b"\n"
    check(uc.without_has_qual(batch), streams, "has_qual == NULL")


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_query_counts_at_the_wave_block_and_scan_edges(nq):
    batch, streams = uc.random_case(200 + nq, nq, read_len=None if nq < 1000 else 24, name_len=None if nq < 1000 else 5, unaligned=0.2)
    text, unaligned = check(batch, streams, nq)
    assert nq < 63 or 0.1 * nq < unaligned < 0.3 * nq


@pytest.mark.parametrize("nq", [64, 257, 4097])
@pytest.mark.parametrize("share", [0.0, 1.0])
def test_no_query_and_every_query_unaligned(nq, share):
    if share == 1.0:
        batch, streams = uc.random_case(300 + nq, nq, read_len=None if nq < 1000 else 24, name_len=5, unaligned=1.0)
        text, unaligned = check(batch, streams, (nq, share))
        assert unaligned == nq and len(text) > 30 * nq
    else:
        plain, _ = sc.all_unaligned_case(nq)
        batch = uc.with_qualities(plain, 9)
        assert check(batch, sm.none_unaligned_case(nq), (nq, share)) == (b"", 0)


def test_record_ends_on_both_sides_of_the_tile_multiples():
    tile = _capi.lib().xm_sam_tile_bytes()
    batch, streams, ends = uc.tile_edge_case(tile)
    text, _ = check(batch, streams, "tile edges")
    assert len(ends) == 9 and all(text[e - 1:e] == b"\n" for e in ends) and sorted(set(e % tile for e in ends)) == [0, 1, tile - 1]


def test_one_unaligned_query_between_4096_aligned_ones():
    batch, streams = uc.one_between(4097, 2048)
    text, unaligned = check(batch, streams, "one between")
    assert unaligned == 1 and text.startswith(b"@q2048\n") and len(text) == 1 + 5 + 1 + 150 + 1 + 2 + 150 + 1


def test_no_query_at_all_launches_nothing():
    batch, streams = uc.random_case(1, 3)
    text, mates, kernel_ms = gpu_unaligned(batch, streams, nq=0)
    assert text == b"" and mates == 0 and kernel_ms == 0


SAM_ONLY = {"mate_beyond_the_query", "third_component", "pair_with_one_sequence"}  # formatRange accepts them when it writes no SAM (tests/test_summary_rules.py)


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_a_malformed_slice_fails_with_the_query_named_and_the_next_call_works(name):
    batch, streams, _ = sc.malformed_cases()[name]
    batch = uc.with_qualities(batch, 5)
    lowest = 4 if name in SAM_ONLY else 2   # (as xm_summary_last: query 2 only where the host rejects it without a SAM file)
    with pytest.raises(RuntimeError, match="malformed result streams"):
        uc.expected(batch, streams)
    with pytest.raises(RuntimeError, match="malformed result streams: query %d$" % lowest):
        gpu_unaligned(batch, streams)
    check(*uc.random_case(5, 300), "after the error")


# ---------------------------------------------------------------- real alignments
N_READS = 2000


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    """The reference of unaligned_cases.real_reference, 2 000 single reads and 1 000 pairs of 100 to 150 bases of which every fifth is random, as FASTQ with
    qualities and (the singles) as FASTA wrapped at 60 letters; a database with the contig names set."""
    d = tmp_path_factory.mktemp("unaligned_real")
    contigs = uc.real_reference()
    singles, pairs = uc.real_reads(N_READS, seed=41), uc.real_reads(N_READS // 2, seed=42, pairs=True)
    files = {k: str(d / k) for k in ("se.fq", "se.fa", "p1.fq", "p2.fq", "ref.fa")}
    open(files["se.fq"], "wb").write(uc.fastq_text(singles, 0, "single%d", 1))
    open(files["se.fa"], "wb").write(uc.fasta_text(singles, 0, "single%d"))
    open(files["p1.fq"], "wb").write(uc.fastq_text(pairs, 0, "pair%d/1", 2))
    open(files["p2.fq"], "wb").write(uc.fastq_text(pairs, 1, "pair%d/2", 3))
    open(files["ref.fa"], "wb").write(b"".join(b">" + n.encode() + b"\n" + uc.DEC[c].tobytes() + b"\n" for n, c in contigs))
    db = api.ReferenceDatabase(contigs)
    names = [n for n, _ in contigs]
    db.set_sam_contigs(names)
    yield {"db": db, "names": names, "files": files}
    db.close()


BLOCKS = {
    "singles": lambda f, size: hostio.read_text_blocks(f["se.fq"], None, size, keep_qualities=True),
    "pairs": lambda f, size: hostio.read_text_blocks(f["p1.fq"], f["p2.fq"], size, keep_qualities=True, expected_inner=100.0, deviation=50.0),
    "wrapped_fasta": lambda f, size: hostio.read_text_blocks(f["se.fa"], None, size, keep_qualities=True, fasta=True),
    "split": lambda f, size: hostio.read_text_blocks(f["se.fq"], None, size, keep_qualities=True, split=60),
}


def written(names, batch, result, **kw):
    """What hostio.Writer makes of the batch -> (SAM bytes, the unaligned-query file, the five statistics bit for bit)."""
    with tempfile.TemporaryFile("w+b") as sam, tempfile.TemporaryFile("w+b") as un:
        w = hostio.Writer(names, sam, un, threads=2)
        w.write(batch, result, **kw)
        sam.seek(0); un.seek(0)
        return sam.read(), un.read(), uc.stats_bits(w.stats)


SIX = ("codes", "names", "name_off", "quals", "qual_off", "has_qual")


@pytest.mark.parametrize("which", sorted(BLOCKS))
def test_a_job_that_leaves_batch_and_streams_in_hbm_writes_what_the_host_writes(real, which):
    db, names = real["db"], real["names"]
    try:
        # 1. both copies on, the host writer: the yardstick - and already here the GPU's text of the unaligned queries equals the host's
        (block,) = BLOCKS[which](real["files"], 1_000_000)
        db.stage_fastq(block)
        assert all(getattr(block._staged.contents, k) for k in SIX) and block.on_host
        db.commit_staged()
        r = db.align_resident(PARAMS)
        want = written(names, block, r)
        summary = sm.recount((r.ints, r.dbls, r.int_off, r.dbl_off), num_contigs=1)
        assert 0.10 * len(block) <= summary.num_unaligned <= 0.50 * len(block)   # (from the host path's streams; a fifth by construction)
        assert len(block) == {"singles": N_READS, "pairs": N_READS // 2, "wrapped_fasta": N_READS}.get(which, len(block)) and (which != "split" or len(block) > 2 * N_READS)
        text = db.unaligned_format_last()
        assert bytes(text) == want[1] and text.records == summary.num_unaligned * (2 if which == "pairs" else 1) and text.kernel_ms > 0 and text.h2d_ms == 0
        text.close()
        # (FASTQ mates with their qualities; FASTA mates, and the sections of a split size, which carry none)
        assert (want[1].count(b"\n+\n") >= summary.num_unaligned) if which in ("singles", "pairs") else (want[1].startswith(b">") and b"\n+\n" not in want[1])
        block.close()
        # 2. neither copy: the three calls and the writer that only writes
        db.set_batch_copy(False)
        db.set_result_copy(False)
        (block,) = BLOCKS[which](real["files"], 1_000_000)
        db.stage_fastq(block)
        staged = block._staged.contents
        assert not any(getattr(staged, k) for k in SIX) and staged.codes_length > 100 * len(block) // (3 if which == "split" else 1) and staged.kernel_ms > 0
        assert block.codes is None and block.on_host is False
        with pytest.raises(ValueError, match="stayed in HBM"):
            block[0]
        db.commit_staged()
        r = db.align_resident(PARAMS)
        assert r.int_off is None
        sam, summary, un = db.format_sam_last(), db.summary_last(), db.unaligned_format_last()
        assert len(summary.unaligned) == 0
        with pytest.raises(ValueError, match="the text must be given"):
            written(names, block, r, sam_text=sam, summary=summary)
        assert written(names, block, r, sam_text=sam, summary=summary, unaligned_text=un) == want
        for held in (sam, summary, un, block):
            held.close()
    finally:
        db.set_batch_copy(True)
        db.set_result_copy(True)
        db.unstage()


PINNED_PROBE = """
import sys
sys.path[:0] = [%r, %r]
import unaligned_cases as uc
from mapper_amd import _capi, api, hostio
db = api.ReferenceDatabase(uc.real_reference())
held = []
for copy in (False, True):
    db.set_batch_copy(copy)
    before = _capi.pinned_host_bytes()[0]
    (block,) = hostio.read_text_blocks(sys.argv[1], None, 1000000, keep_qualities=True)
    db.stage_fastq(block)
    held.append(block)  # (its buffers stay in use: the next staging call cannot take them over)
    print("pinned", int(copy), _capi.pinned_host_bytes()[0] - before, int(block._staged.contents.codes_length))
for block in held:
    block.close()
db.close()
"""


def test_staging_without_the_copy_takes_less_pinned_memory(real):
    """In a process of its own, whose pool of pinned buffers is empty at the start: what a staging call adds to xm_pinned_host_bytes with the copy off - the
    mate counts, offsets and lengths: 4 + 16 + 8 bytes a query - and with it on, the six other arrays beside them."""
    r = subprocess.run([sys.executable, "-c", PINNED_PROBE % (ROOT, os.path.join(ROOT, "tests")), real["files"]["se.fq"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [line.split() for line in r.stdout.splitlines() if line.startswith("pinned")]
    (_, off_flag, off_bytes, codes), (_, on_flag, on_bytes, _) = lines
    off_bytes, on_bytes, codes = int(off_bytes), int(on_bytes), int(codes)
    assert (off_flag, on_flag) == ("0", "1") and codes > 100 * N_READS
    assert 28 * N_READS <= off_bytes < 2 * 28 * N_READS + 3 * 4096   # (the pool gives an eighth more than asked)
    assert on_bytes > off_bytes + 2 * codes                          # (codes and qualities, a byte a base each, and the names and offsets on top)


def test_the_qualities_belong_to_the_batch_they_came_with(real):
    db, names = real["db"], real["names"]
    a, b = BLOCKS["singles"](real["files"], N_READS // 2)
    try:
        db.stage_fastq(a)
        db.commit_staged()
        db.stage_fastq(b)               # B, with other names and qualities, is staged while A is resident
        ra = db.align_resident(PARAMS)
        ta = db.unaligned_format_last()
        want = written(names, a, ra)[1]
        assert bytes(ta) == want and want.startswith(b"@single4\n") and b"@single%d\n" % (N_READS // 2 + 4) not in want and want.count(b"\n+\n") >= N_READS // 10
        ta.close()
        db.commit_staged()
        with pytest.raises(RuntimeError, match="no longer resident"):
            db.unaligned_format_last()
        rb = db.align_resident(PARAMS)
        tb = db.unaligned_format_last()
        want_b = written(names, b, rb)[1]
        assert bytes(tb) == want_b and want_b.startswith(b"@single%d\n" % (N_READS // 2 + 4)) and want_b != want
        tb.close()
    finally:
        a.close(); b.close()
        db.unstage()


def query_batch(queries):
    import oracle_lib as o
    b = o.QueryBatch(queries)
    return b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation


def test_what_the_call_refuses():
    contigs, _ = pg.reference()
    ordinary = pg.ordinary_queries(300)
    contained = pg.one_of_each_kind()["contained"][0]   # a mate inside its partner: the reference would have thrown
    db = api.ReferenceDatabase(contigs)
    try:
        # a batch staged from arrays has no names in HBM
        db.upload_arrays(*query_batch(ordinary))
        db.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match="xm_unaligned_format_last: the resident batch has no names in HBM"):
            db.unaligned_format_last()
        db.stage_arrays(*query_batch(ordinary[:100]))
        db.commit_staged()
        with pytest.raises(RuntimeError, match="no longer resident"):
            db.unaligned_format_last()
        # an align call that fails
        db.upload_arrays(*query_batch(pg.with_throwers(ordinary, [(120, contained)])))
        with pytest.raises(RuntimeError, match="Failed to align query 120"):
            db.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match="no longer resident"):
            db.unaligned_format_last()
    finally:
        db.close()


# ---------------------------------------------------------------- the command line
def run_job(argv, out_dir, outputs):
    os.makedirs(out_dir)
    log = io.StringIO()
    assert cli.run(argv + [x for flag, name in outputs for x in (flag, str(out_dir / name))], out=log) == 0
    text = log.getvalue()
    return tuple(open(out_dir / name, "rb").read() for _, name in outputs) + (text[text.index("Statistics"):],)


GPU_FLAGS = ["--parse-on-gpu", "--results-on-gpu"]
BOTH = ["--unaligned-on-gpu", "--batch-on-gpu"]


@pytest.mark.parametrize("contexts", [["--contexts", "2"], ["--devices", "0,0"], ["--contexts", "1"]])
def test_command_line_writes_the_same_bytes_with_the_two_flags(real, tmp_path, contexts):
    """Five batches.  --contexts 2 and --devices 0,0: through MultiGpuDatabase, two contexts on GPU 0; --contexts 1: through one ReferenceDatabase."""
    base = ["--reference", real["files"]["ref.fa"], "--queries", real["files"]["se.fq"], "--batch-size", str(N_READS // 5 + 1)] + contexts + GPU_FLAGS + ["--format-on-gpu"]
    outputs = (("--out-sam", "sam"), ("--out-unaligned", "unaligned"))
    plain = run_job(base, tmp_path / "plain", outputs)
    assert len(plain[0]) > 100_000 and plain[1].count(b"\n+\n") == N_READS // 5 and plain[1].startswith(b"@single4\n") and "Alignment rate                : 80% of queries" in plain[2]
    assert run_job(base + BOTH, tmp_path / "both", outputs) == plain
    assert run_job(base + ["--unaligned-on-gpu"], tmp_path / "text", outputs) == plain


def test_command_line_mutations_with_the_batch_in_hbm(real, tmp_path):
    """The pile-up must not need the host's batch: --out-mutations without --out-sam and --format-on-gpu."""
    contigs, batches = pw.three_batches()
    reads = [(m[0],) for b in batches for m in pw.mates_of(b)]
    open(tmp_path / "ref.fa", "wb").write(b"".join(b">" + n.encode() + b"\n" + uc.DEC[c].tobytes() + b"\n" for n, c in contigs))
    open(tmp_path / "se.fq", "wb").write(uc.fastq_text(reads, 0, "read%d", 4))
    base = ["--reference", str(tmp_path / "ref.fa"), "--queries", str(tmp_path / "se.fq"), "--batch-size", "150", "--contexts", "2"] + GPU_FLAGS
    outputs = (("--out-mutations", "mutations"), ("--out-unaligned", "unaligned"))
    plain = run_job(base, tmp_path / "plain", outputs)
    assert len(reads) == 741 and len(plain[0]) > 0 and plain[1].count(b"\n+\n") >= 40
    assert run_job(base + BOTH, tmp_path / "both", outputs) == plain


@pytest.mark.parametrize("flags,message", [
    (["--out-unaligned", "u.fq", "--unaligned-on-gpu", "--results-on-gpu"], "--unaligned-on-gpu needs --parse-on-gpu"),
    (["--no-output", "--unaligned-on-gpu", "--parse-on-gpu", "--results-on-gpu"], "--unaligned-on-gpu has nothing to do without --out-unaligned"),
    (["--out-unaligned", "u.fq", "--batch-on-gpu", "--parse-on-gpu", "--results-on-gpu"], "--batch-on-gpu with --out-unaligned needs --unaligned-on-gpu"),
    (["--no-output", "--batch-on-gpu", "--per-object"], "--batch-on-gpu and --per-object exclude each other"),
])
def test_usage_errors_exit_with_status_1_and_their_message(real, capsys, flags, message):
    assert cli.main(["--reference", real["files"]["ref.fa"], "--queries", real["files"]["se.fq"]] + flags) == 1
    assert "Error: " + message in capsys.readouterr().err
