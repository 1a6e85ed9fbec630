"""GPU tier: SAM records formatted on the GPU (xm_sam_format_last, api.ReferenceDatabase.format_sam_last, `--format-on-gpu`; the kernels of
mapper_amd/csrc/xm_sam.h over the rules of xm_sam_rules.h).  The yardstick everywhere is the host formatter: every text equals hostio.Writer's bytes for the
same batch and streams, every double hostio.java_double's string - at the edges of the wavefront, the scan block and the write kernel's tile; a malformed
slice fails the call with the query named and leaves the device usable; the names belong to the batch they came with; the command line writes the same
bytes with and without the flag."""
import ctypes as C
import io
import os
import tempfile

import numpy as np
import pytest

import pileup_workloads as pw
import sam_cases as sc
from mapper_amd import _capi, api, cli, hostio, synth

pytestmark = pytest.mark.gpu
PARAMS = api.AlignmentParameters()
DEC = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)


def gpu_format(batch, streams, contigs=sc.CONTIGS):
    """xm_test_sam_format on a sam_cases batch and streams -> (text, records); RuntimeError with the library's message."""
    L = _capi.lib()
    ints, dbls, io_, do = streams.arrays() if isinstance(streams, sc.Streams) else streams
    names = (C.c_char_p * len(contigs))(*[c.encode() for c in contigs])
    raw = batch._raw
    job = _capi.XmTestSamJob(batch.num_queries, batch.mate_count.ctypes.data, batch.mate_offset.ctypes.data, batch.mate_length.ctypes.data, batch.codes.ctypes.data, batch.codes_length,
                             raw.names, batch.name_off.ctypes.data, len(contigs), 0, names, ints.ctypes.data, dbls.ctypes.data, io_.ctypes.data, do.ctypes.data)
    out = C.POINTER(_capi.XmSamText)()
    if L.xm_test_sam_format(0, C.byref(job), C.byref(out)):
        assert not out
        raise RuntimeError(L.xm_last_error().decode())
    t = api.SamText(L, out)
    assert t.h2d_ms >= 0 and t.kernel_ms > 0 and t.d2h_ms >= 0
    text, records = bytes(t), t.records
    t.close()
    return text, records


def check(batch, streams, what=""):
    want = sc.expected(batch, streams)
    text, records = gpu_format(batch, streams)
    assert records == want.count(b"\n"), what
    if text != want:
        at = next(i for i in range(min(len(text), len(want)) + 1) if text[i:i + 1] != want[i:i + 1])
        raise AssertionError("%s: %d bytes, %d wanted; first difference at byte %d: %r / %r" % (what, len(text), len(want), at, text[max(at - 40, 0):at + 40], want[max(at - 40, 0):at + 40]))
    return want


# ---------------------------------------------------------------- Double.toString
def double_corpus():
    rng = np.random.default_rng(12)
    p2 = np.ldexp(1.0, np.arange(-1074, 1024))
    p10 = np.array([float("1e%d" % k) for k in range(-323, 309)])
    base = np.concatenate([p2, p10])
    inf = np.full(len(base), np.inf)
    edges = np.array([5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308, 9999999.999999998, 1.0e7, 0.001, 9.999999999999999e-4, -0.0, 0.0,
                      float("nan"), float("inf"), float("-inf"), 0.6000000000000001, 7.300000000000001, -2.5])
    rand = rng.integers(0, 2**64, 200_000, dtype=np.uint64).view(np.float64)
    counts = [rng.integers(0, hi, 200_000) for hi in (12, 12, 12, 26, 26)]  # a * 1 + b * 1.5 + c * 0.5 + d * 0.6 + e * 0.1, added up in that order
    sums = np.zeros(200_000)
    for n, step in zip(counts, (1.0, 1.5, 0.5, 0.6, 0.1)):
        for i in range(int(n.max())):
            sums = np.where(i < n, sums + step, sums)
    return np.concatenate([base, np.nextafter(base, inf), np.nextafter(base, -inf), -base, edges, rand, sums])


def test_doubles_equal_the_host_formatter():
    x = np.ascontiguousarray(double_corpus())
    n = len(x)
    assert n > 400_000
    out = np.zeros(24 * n, np.uint8)
    lens = np.zeros(n, np.int32)
    L = _capi.lib()
    assert L.xm_test_format_doubles(0, n, x.ctypes.data, out.ctypes.data, lens.ctypes.data) == 0, L.xm_last_error()
    assert lens.min() >= 3 and lens.max() <= 24
    raw = out.tobytes()
    for i in range(n):
        got = raw[24 * i:24 * i + lens[i]].decode()
        assert got == hostio.java_double(x[i]), (i, x[i].hex(), got)


# ---------------------------------------------------------------- records from given streams
def test_every_shape():
    batch, streams = sc.shapes_case()
    want = check(batch, streams, "shapes")
    assert want.count(b"\n") == 40 and b"\t2147483648\t" in want and b"4S40M6S" in want and b"10M3I4D5M3D3I30M" in want


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4200])
def test_query_counts_at_the_wave_block_and_scan_edges(nq):
    batch, streams = sc.random_case(100 + nq, nq, read_len=None if nq < 1000 else 24, name_len=None if nq < 1000 else 5, unaligned=0.2 if nq > 1 else 0.0)
    assert len(check(batch, streams, nq)) > 40 * nq  # (the yardstick's own text: most queries have records)


@pytest.mark.parametrize("length", [1, 15, 16, 17, 63, 64, 65, 150, 1000])
def test_read_lengths(length):
    check(*sc.random_case(200 + length, 130, read_len=length), what=length)


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 63, 64, 65])
def test_name_lengths(length):
    check(*sc.random_case(300 + length, 130, name_len=length), what=length)


def test_records_end_on_both_sides_of_the_tile_edges():
    T = _capi.lib().xm_sam_tile_bytes()
    assert T >= 256 and T % 16 == 0
    batch, streams, ends = sc.tile_edge_case(T)
    want = check(batch, streams, "tile edges")
    record_ends = {i + 1 for i, c in enumerate(want) if c == 10}
    assert set(ends) <= record_ends and {e % T for e in ends} == {0, 1, T - 1}


def test_all_unaligned_is_an_empty_text():
    assert gpu_format(*sc.all_unaligned_case(300)) == (b"", 0)


def test_one_query_with_three_alignments():
    assert check(*sc.three_alignments_case()).count(b"\n") == 3


def test_a_malformed_slice_fails_the_call_and_the_next_call_works():
    batch, streams = sc.random_case(77, 300, unaligned=0.0)
    ints, dbls, io_, do = streams.arrays()
    q = next(k for k in range(150, 300) if io_[k + 1] - io_[k] >= 11)       # (a query in the middle with an alignment: its slice holds what is written over it)
    later = next(k for k in range(q + 50, 300) if io_[k + 1] - io_[k] >= 11)
    bad = ints.copy()
    bad[io_[q]:io_[q] + 4] = [1, 1, 17, 3]  # one component, one alignment, of three sequences
    bad[io_[later]:io_[later] + 4] = [1, 1, 17, 0]  # (a second one behind it: the lowest is reported)
    with pytest.raises(RuntimeError, match="malformed result streams"):
        sc.expected(batch, (bad, dbls, io_, do))
    with pytest.raises(RuntimeError) as e:
        gpu_format(batch, (bad, dbls, io_, do))
    assert "malformed result streams" in str(e.value) and str(e.value).endswith("query %d" % q), str(e.value)
    check(batch, (ints, dbls, io_, do), "after the error")


@pytest.mark.parametrize("name", sorted(sc.malformed_cases()))
def test_every_malformed_condition(name):
    batch, streams, q = sc.malformed_cases()[name]
    with pytest.raises(RuntimeError, match="malformed result streams: query %d$" % q):
        gpu_format(batch, streams)


# ---------------------------------------------------------------- the real path
def letters(codes):
    return DEC[codes].tobytes()


def fastq_of(reads, name="r%d"):
    return b"".join(b"@" + (name % i).encode() + b" description\n" + letters(r) + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """Three contigs (pileup_workloads.fallback_pairs), its pairs - at contig ends, where they fall back to one component per mate, and ordinary ones with
    indels, and twenty pairs that align nowhere - and 2 000 single reads with indels plus 100 that align nowhere, as FASTQ files; a database with the contig names set."""
    d = tmp_path_factory.mktemp("sam_real")
    contigs, batches = pw.fallback_pairs()
    elsewhere = synth.synthetic_reference(5_000, seed=98)
    j1, j2 = synth.synthetic_paired_end(elsewhere, 20, seed=53)[:2]
    pairs = pw.mates_of(batches[0])[:980] + [[a, b] for a, b in zip(j1, j2)]  # (the last twenty align nowhere)
    singles = list(synth.synthetic_single_end(contigs[0][1], 2000, seed=51, indel_prob=0.3)[0]) + list(synth.synthetic_single_end(elsewhere, 100, seed=52)[0])
    files = {"se": str(d / "se.fq"), "p1": str(d / "p1.fq"), "p2": str(d / "p2.fq"), "ref": str(d / "ref.fa")}
    open(files["se"], "wb").write(fastq_of(singles, "single%d"))
    open(files["p1"], "wb").write(fastq_of([p[0] for p in pairs], "pair%d/1"))
    open(files["p2"], "wb").write(fastq_of([p[1] for p in pairs], "pair%d/2"))
    open(files["ref"], "wb").write(b"".join(b">" + n.encode() + b"\n" + letters(c) + b"\n" for n, c in contigs))
    db = api.ReferenceDatabase(contigs)
    names = [n for n, _ in contigs]
    db.set_sam_contigs(names)
    yield {"db": db, "names": names, "files": files, "dir": d}
    db.close()


def host_bytes(names, batch, result):
    with tempfile.TemporaryFile("w+b") as f:
        hostio.Writer(names, f, None, threads=2).write(batch, result)
        f.seek(0)
        return f.read()


def text_blocks(files, which, batch_size=1_000_000):
    if which == "se":
        return list(hostio.read_text_blocks(files["se"], None, batch_size))
    return list(hostio.read_text_blocks(files["p1"], files["p2"], batch_size, expected_inner=pw.PAIR_SPACING[0], deviation=pw.PAIR_SPACING[1]))


def host_batches(files, which, batch_size=1_000_000):
    if which == "se":
        return list(hostio.read_batches(files["se"], None, batch_size))
    return list(hostio.read_batches(files["p1"], files["p2"], batch_size, expected_inner=pw.PAIR_SPACING[0], deviation=pw.PAIR_SPACING[1]))


def shapes_of(result, text):
    """What the GPU's own result holds: (unaligned queries, queries of two components with alignments, insertions or deletions in the CIGARs, records on the reverse strand)."""
    io_, ints = result.int_off, result.ints
    nq = len(io_) - 1
    none = [bool((ints[io_[q]] == 1 and ints[io_[q] + 1] == 0) or (ints[io_[q]] == 2 and ints[io_[q] + 1] == 0 and ints[io_[q] + 2] == 0)) for q in range(nq)]  # (a pair without alignments has two empty components)
    unaligned = sum(none)
    fallback = sum(1 for q in range(nq) if ints[io_[q]] == 2 and not none[q])
    fields = [line.split(b"\t") for line in text.split(b"\n")[:-1]]
    indels = sum(1 for f in fields if b"I" in f[5] or b"D" in f[5])
    reverse = sum(1 for f in fields if int(f[1]) & 16)
    return unaligned, fallback, indels, reverse


@pytest.mark.parametrize("which", ["se", "pairs"])
def test_staged_fastq_formats_as_the_host_does(work, which):
    db = work["db"]
    (block,) = text_blocks(work["files"], which)
    db.stage_fastq(block)
    db.commit_staged()
    r = db.align_resident(PARAMS)
    t = db.format_sam_last()
    want = host_bytes(work["names"], block, r)
    assert bytes(t) == want and t.records == want.count(b"\n") and t.kernel_ms > 0
    t.close()
    unaligned, fallback, indels, reverse = shapes_of(r, want)
    if which == "se":
        assert len(block) == 2100 and unaligned >= 90 and indels > 300 and reverse > 500 and b"single7 description" not in want and b"single7\t" in want
    else:
        assert len(block) == 1000 and fallback > 30 and indels > 100 and reverse > 300 and unaligned >= 15
    block.close()


@pytest.mark.parametrize("which", ["se", "pairs"])
def test_staged_arrays_with_the_hosts_names_format_as_the_host_does(work, which):
    db = work["db"]
    (batch,) = host_batches(work["files"], which)
    db.stage_arrays(*batch.arrays())
    db.commit_staged()
    r = db.align_resident(PARAMS)
    t = db.format_sam_last(batch)
    want = host_bytes(work["names"], batch, r)
    assert bytes(t) == want and len(want) > 100_000
    t.close()
    with pytest.raises(RuntimeError, match="no names in HBM"):  # staged from arrays: no names were given
        db.format_sam_last()
    batch.close()


def test_the_names_belong_to_the_batch_they_came_with(work):
    db = work["db"]
    a, b = text_blocks(work["files"], "se", 1050)
    db.stage_fastq(a)
    db.commit_staged()
    db.stage_fastq(b)               # B is staged while A is resident
    ra = db.align_resident(PARAMS)
    ta = db.format_sam_last()
    want = host_bytes(work["names"], a, ra)
    assert bytes(ta) == want and b"single0\t" in want and b"single1050\t" not in want
    ta.close()
    db.commit_staged()
    with pytest.raises(RuntimeError, match="no longer resident"):
        db.format_sam_last()
    rb = db.align_resident(PARAMS)
    tb = db.format_sam_last()
    want = host_bytes(work["names"], b, rb)
    assert bytes(tb) == want and b"single1050\t" in want and b"single0\t" not in want
    tb.close()
    a.close(); b.close()


def test_a_context_without_contig_names_is_an_error(work):
    c = work["db"].new_context()
    try:
        (batch,) = host_batches(work["files"], "se")
        c.upload_arrays(*batch.arrays())
        c.align_resident(PARAMS)
        with pytest.raises(RuntimeError, match="xm_sam_set_contigs"):
            c.format_sam_last(batch)
        with pytest.raises(RuntimeError, match="2 names for an index of 3 contigs"):
            c.set_sam_contigs(work["names"][:2])
        batch.close()
    finally:
        c.close()


# ---------------------------------------------------------------- the command line
JOBS = {
    "single_three_batches": lambda f: ["--queries", f["se"], "--batch-size", "700"],
    "pairs": lambda f: ["--paired-queries", f["p1"], f["p2"], "--spacing", "100", "50"],
}


@pytest.mark.parametrize("name", sorted(JOBS))
def test_command_line_writes_the_same_bytes_with_the_flags(work, tmp_path, name):
    runs = {}
    for parse in (False, True):
        for fmt in (False, True):
            out_dir = tmp_path / ("parse%d_format%d" % (parse, fmt))
            os.makedirs(out_dir)
            argv = ["--reference", work["files"]["ref"]] + JOBS[name](work["files"]) + ["--out-sam", str(out_dir / "sam"), "--out-unaligned", str(out_dir / "unaligned")]
            argv += (["--parse-on-gpu"] if parse else []) + (["--format-on-gpu"] if fmt else [])
            log = io.StringIO()
            assert cli.run(argv, out=log) == 0
            text = log.getvalue()
            phases = cli.last_timing["phases"]
            assert sorted(phases) == ["align", "format", "read", "stage", "write"] and all(v >= 0 for v in phases.values()) and phases["align"] > 0 and phases["format"] > 0
            runs[(parse, fmt)] = (open(out_dir / "sam", "rb").read(), open(out_dir / "unaligned", "rb").read(), text[text.index("Statistics"):])
    first = runs[(False, False)]
    assert len(first[0]) > 100_000 and first[0].startswith(b"@HD") and first[1].count(b"\n+\n") >= (90 if name != "pairs" else 2)
    for key, got in runs.items():
        assert got == first, key
