"""The last lines of every pass of xm_align_batch on the GPU: room in the two result arenas (publishRead, mapper_amd/csrc/xm_kernel_common.h; its copies in
xm_wave_kernel.hip and xm_memo_replay_kernel), the rerun of the reads that found an arena full (PassKind::OutRerun: runLanePasses grows both arenas with
ResultStage::growAfterOverflow and runs the `out` list in front of whatever else is pending), and the scan and gather that turn per-read lengths into the query-order streams
(xm_scan_*_kernel, xm_gather_kernel, xm_collapse_fanout_kernel; ResultStage::toHost, mapper_amd/csrc/xm_result_stage.h).

The arenas are per context and only ever grow, so the overflow path runs on the first call of a context whose reads have many alignments and never again:
every overflow case takes a fresh context (db.new_context(): the tables are shared) and proves from the pass trace (XM_TRACE_PASSES=1, as
tests/test_gpu_dense_waves.py reads it) that the path ran - which pass reported `out`, that the next pass ran exactly those reads, that none reported it later.
A case that passes without the overflow fails on those asserts.

Reference.  The oracle aligns a small set U of distinct queries once per module (helpers.align_each: streams, and every query's own contribution to the
counters from one-query calls); a test batch is a sequence of indices into U (helpers.compose_batch) and what it must give is put together in numpy
(helpers.compose_streams).  Every comparison is bit for bit.  U is cut from pileup_workloads.family_reference: families of k exact copies of a 400-base segment,
so that one 150-base read gives k alignments - 2 + 9k ints and 6k doubles where a query without alignments gives 2 and 0."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import oracle_lib as o
from helpers import streams_equal, first_difference, compose_batch, compose_streams, align_each
from pileup_workloads import FAMILY_SIZES, CODES, family_reference, fragment_pair, with_indel, rc, single
from mapper_amd import api

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count())
MEMO = 64 << 20


# the arenas a context's first call of nq queries starts with (xm_pass_plan.h, firstArenaSize: ResultStage::reserveArenas) and what a rerun grows them to
# (grownArenaSize: ResultStage::growAfterOverflow).  Written once here, independently of them (tests/test_pass_plan.py holds the two against each other): the cases below are sized by them, and assert from the oracle's lengths that they still overflow.
def initial_int_cap(nq):
    return nq * 40 + 4096


def initial_dbl_cap(nq):
    return nq * 12 + 4096


def grown_cap(cap, cursor):
    return max(4 * cap + 65536, 2 * cursor)


Pass = namedtuple("Pass", "number kind reads scale lanes_per_read filter heavy rescale out")
PASS = re.compile(r"\[xm\] pass (\d+): (light|gapped) reads (\d+) scale (\d+) lpw \d+ waves \d+ lanes/read (\d+) filter (\d): [0-9.]+ ms -> heavy (\d+) scale (\d+) out (\d+)")
WAVE = re.compile(r"\[xm\] wave tier (\d+) config \d+: reads (\d+), .*lane-per-read (\d+) \(so far\)")


def run_traced(ctx, b, capfd, monkeypatch, **env):
    """One call -> (result, [Pass] of its lane-per-read passes in order, [(tier, reads, lane-per-read so far)] of its wave tiers)."""
    monkeypatch.setenv("XM_TRACE_PASSES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    try:
        got = ctx.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())
    finally:
        err = capfd.readouterr().err
        for k in env:
            monkeypatch.delenv(k)
    passes = [Pass(int(m.group(1)), m.group(2), *(int(x) for x in m.groups()[2:])) for m in PASS.finditer(err)]
    return got, passes, [tuple(int(x) for x in m.groups()) for m in WAVE.finditer(err)]


def overflowed(passes, kinds):
    """The passes that reported `out` are of `kinds`, in that order (none later); each is followed by a pass of the same kind and scale over exactly those
    reads.  -> their indices in `passes`."""
    at = [i for i, p in enumerate(passes) if p.out > 0]
    assert [passes[i].kind for i in at] == list(kinds), ("passes that found a result arena full", kinds, passes)
    for i in at:
        assert i + 1 < len(passes), passes
        p, nxt = passes[i], passes[i + 1]
        assert (nxt.reads, nxt.kind, nxt.scale) == (p.out, p.kind, p.scale), ("the rerun of the reads that found the arena full", passes)
    return at


def expected_counters(want, filter_ran=False):
    """counters[:8] as tests/test_gpu_parity.py compares them with the oracle's; with the rejection filter, without the work it skipped (test_gpu_dense_waves.work_counters)."""
    wc = [int(x) for x in want.counters]
    skipped_calls = wc[16] if filter_ran else 0
    skipped_nodes = wc[12] + wc[17] if filter_ran else 0
    return [wc[0], wc[1] + wc[2], wc[2], wc[3], wc[5], wc[6] - skipped_calls, wc[7] - skipped_nodes, wc[8]]


def check_result(got, want, nq, filter_ran=False):
    assert streams_equal(want, got), first_difference(want, got, nq)
    assert (len(got.ints), len(got.dbls)) == (int(want.int_off[-1]), int(want.dbl_off[-1]))
    assert [int(x) for x in got.counters[:8]] == expected_counters(want, filter_ran)
    assert int(got.counters[8]) == want.alignments_out


def lengths(want, idx):
    """(ints, doubles) the queries idx of U put into the arenas, summed."""
    idx = np.asarray(idx, np.int64)
    return int((want.int_off[idx + 1] - want.int_off[idx]).sum()), int((want.dbl_off[idx + 1] - want.dbl_off[idx]).sum())


# ---------------------------------------------------------------- U

class Universe:
    """contigs, U (an oracle_lib.QueryBatch), cls: {class name: indices into U}, want: the oracle's run over U (helpers.align_each)."""


def family_reads(seq, n, rng, deletion):
    """n distinct 150-base reads from inside a family's 400-base segment, either strand; `deletion`: with a 3-base deletion away from the ends."""
    picks = rng.permutation(2 * (len(seq) - 153))[:n]
    out = []
    for p in picks:
        start, reverse = int(p) // 2, bool(p & 1)
        read = with_indel(seq[start:start + 153], 150, int(rng.integers(40, 110)), 3 if deletion else 0, rng)
        out.append(single(rc(read) if reverse else read))
    return out


def short_universe(seed=0x0F10):
    rng = np.random.default_rng([seed, 1])   # (family_reference draws the families from default_rng(seed))
    contigs, families = family_reference((70_000, 45_000, 25_000), FAMILY_SIZES, seed)
    in_family = [np.zeros(len(r), bool) for _, r in contigs]
    for seq, places in families.values():
        for c, at, _ in places:
            in_family[c][max(0, at - 400):at + 800] = True
    classes = {"a23": family_reads(families[23][0], 320, rng, False), "a5": family_reads(families[5][0], 150, rng, False),
               "b23": family_reads(families[23][0], 160, rng, True), "c": [], "d": [single(CODES[rng.integers(0, 4, 150)]) for _ in range(40)], "e": []}
    while len(classes["c"]) < 60 or len(classes["e"]) < 6:
        c = int(rng.integers(0, len(contigs)))
        start = int(rng.integers(0, len(contigs[c][1]) - 400))
        if in_family[c][start]:
            continue
        region = contigs[c][1][start:start + 400]
        if len(classes["c"]) < 60:
            classes["c"].append(single(rc(region[:150]) if start & 1 else region[:150].copy()))
        else:
            classes["e"].append(fragment_pair(region, 40, rng, reverse=bool(start & 1)))
    return contigs, classes


def long_universe(seed=0x0F1F):
    rng = np.random.default_rng([seed, 1])   # (family_reference draws the families from default_rng(seed))
    contigs, families = family_reference((60_000, 40_000), (11,), seed, segment=1400, slot=2000)
    seq = families[11][0]
    out = []
    for p in rng.permutation(2 * (len(seq) - 1003))[:100]:
        # (a 3-base deletion in each: an exact read could be finished by the light pass, and the case is about the gapped pass's lanes)
        read = with_indel(seq[int(p) // 2:int(p) // 2 + 1003], 1000, int(rng.integers(200, 800)), 3, rng)
        out.append(single(rc(read) if p & 1 else read))
    return contigs, {"f": out}


def make_universe(contigs, classes, observe):
    s = Universe()
    s.contigs, s.cls, queries = contigs, {}, []
    for name, qs in classes.items():
        s.cls[name] = np.arange(len(queries), len(queries) + len(qs))
        queries += qs
    s.U = o.QueryBatch(queries)
    R = o.OracleReference(contigs)
    if observe:
        with o.observe_bound():
            s.want = align_each(R, s.U, o.make_params(), threads=THREADS)
    else:
        s.want = align_each(R, s.U, o.make_params(), threads=THREADS)
    s.int_len, s.dbl_len = np.diff(s.want.int_off), np.diff(s.want.dbl_off)
    return s


@pytest.fixture(scope="module")
def short():
    s = make_universe(*short_universe(), observe=False)
    # the slice lengths the cases are sized by, from the oracle's streams
    for name, k in (("a23", 23), ("a5", 5)):
        assert set(s.int_len[s.cls[name]]) == {2 + 9 * k} and set(s.dbl_len[s.cls[name]]) == {6 * k}, name
    assert set(s.dbl_len[s.cls["b23"]]) == {6 * 23} and s.int_len[s.cls["b23"]].min() >= 2 + 13 * 23   # (two blocks or more per alignment)
    assert set(s.int_len[s.cls["c"]]) == {11} and set(s.dbl_len[s.cls["c"]]) == {6}
    assert set(s.int_len[s.cls["d"]]) == {2} and set(s.dbl_len[s.cls["d"]]) == {0}
    assert s.dbl_len[s.cls["e"]].min() >= 8
    s.db = api.ReferenceDatabase(s.contigs)
    yield s
    s.db.close()


@pytest.fixture(scope="module")
def long_reads():
    s = make_universe(*long_universe(), observe=True)
    assert s.dbl_len[s.cls["f"]].min() >= 6 * 11
    s.db = api.ReferenceDatabase(s.contigs, max_query_length=1000)
    yield s
    s.db.close()


def shuffled(rng, *parts):
    idx = np.concatenate([np.asarray(p, np.int64) for p in parts])
    return idx[rng.permutation(len(idx))]


def case1_indices(s):
    """300 reads of 23 alignments each, a handful of reads with one and with none, four pairs: all distinct."""
    return shuffled(np.random.default_rng(0xC1), s.cls["a23"][:300], s.cls["c"][:12], s.cls["d"][:12], s.cls["e"][:4])


def assert_overflows_both(s, idx, nq=None):
    ni, nd = lengths(s.want, idx)
    nq = len(idx) if nq is None else nq
    assert ni > initial_int_cap(nq) and nd > initial_dbl_cap(nq), ("resize the case: the arenas a fresh context starts with hold this batch", ni, nd, nq)


# ---------------------------------------------------------------- a result arena full

def test_light_pass_overflows_both_arenas(short, capfd, monkeypatch):
    """Case 1.  The light pass of a fresh context fills both arenas; then the same batch on the same context, warm: no pass reports `out`, and the streams and
    counters[0:11] are the first call's (a read that found the arena full used to have its PathAligner calls and nodes counted twice: xm_align_kernel, local = before)."""
    idx = case1_indices(short)
    assert_overflows_both(short, idx)
    b, want = compose_batch(short.U, idx), compose_streams(short.want, idx)
    ctx = short.db.new_context()
    try:
        cold, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        assert passes[0].kind == "light" and passes[0].reads == len(idx)
        assert overflowed(passes, ["light"]) == [0]
        check_result(cold, want, len(idx))
        warm, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        overflowed(passes, [])
        check_result(warm, want, len(idx))
        assert streams_equal(cold, warm)
        assert [int(x) for x in warm.counters[:11]] == [int(x) for x in cold.counters[:11]]
    finally:
        ctx.close()


def test_doubles_only(short, capfd, monkeypatch):
    """Case 2.  Reads of five alignments: 47 ints and 30 doubles each against 40 and 12 per query of room, and the 4 096 spare cover the ints only.  Reads
    without alignments (no doubles) are mixed in: the ones published after the double arena filled up reserve nothing in it and are turned away all the same."""
    rng = np.random.default_rng(0xC2)
    idx = shuffled(rng, short.cls["a5"], short.cls["a5"], short.cls["d"][:30])   # (every read of five alignments twice: nothing collapses here)
    ni, nd = lengths(short.want, idx)
    assert ni <= initial_int_cap(len(idx)) and nd > initial_dbl_cap(len(idx)), ("resize the case: the ints must fit and the doubles must not", ni, nd, len(idx))
    b, want = compose_batch(short.U, idx), compose_streams(short.want, idx)
    ctx = short.db.new_context()
    try:
        got, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        assert overflowed(passes, ["light"]) == [0]
        check_result(got, want, len(idx))
    finally:
        ctx.close()


@pytest.mark.parametrize("env", [{}, {"XM_HANDOVER": "0"}, {"XM_PAIR_LANES": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_gapped_pass_overflows_after_saved_regions(short, env, capfd, monkeypatch):
    """Case 3.  Only reads with a deletion (they stop in front of the gapped chain and keep their seeding state in a region) beside reads with one alignment:
    the light pass publishes little, the gapped pass consumes the saved regions and fills the arenas; its rerun is a gapped pass at the same scale, plain."""
    rng = np.random.default_rng(0xC3)
    gapped, rest = short.cls["b23"][:120], short.cls["c"][:40]
    idx = shuffled(rng, gapped, rest)
    li, ld = lengths(short.want, rest)
    assert li <= initial_int_cap(len(idx)) and ld <= initial_dbl_cap(len(idx))
    assert_overflows_both(short, gapped, len(idx))
    b, want = compose_batch(short.U, idx), compose_streams(short.want, idx)
    ctx = short.db.new_context()
    try:
        got, passes, _ = run_traced(ctx, b, capfd, monkeypatch, **env)
        assert passes[0].kind == "light" and passes[0].heavy > 0 and passes[0].out == 0, passes
        assert passes[1].kind == "gapped" and passes[1].reads == passes[0].heavy and passes[1].lanes_per_read == (1 if "XM_PAIR_LANES" in env else 2), passes
        assert overflowed(passes, ["gapped"]) == [1]
        assert passes[2].scale == passes[1].scale > passes[0].scale, passes
        check_result(got, want, len(idx))
    finally:
        ctx.close()


def test_eight_lanes_per_read(long_reads, capfd, monkeypatch):
    """Case 4.  1 000-base reads of eleven alignments each: the gapped pass runs the rejection filter with eight lanes per read (the first of them publishes)."""
    s = long_reads
    rng = np.random.default_rng(0xC4)
    idx = shuffled(rng, s.cls["f"], s.cls["f"])
    assert_overflows_both(s, idx)
    b, want = compose_batch(s.U, idx), compose_streams(s.want, idx)
    ctx = s.db.new_context()
    try:
        got, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        at = overflowed(passes, ["gapped"])
        assert passes[at[0]].lanes_per_read == 8 and passes[at[0]].filter == 1 and passes[at[0] + 1].lanes_per_read == 8, passes
        assert got.extra[3] == 1
        check_result(got, want, len(idx), filter_ran=True)
    finally:
        ctx.close()


def test_twice_in_one_call(short, capfd, monkeypatch):
    """Case 5.  The light pass fills the arenas, and the gapped pass fills the ones grown after it: the `out` list is double-buffered (nextPass, st.to ^= 1),
    and the second growKeep keeps what two passes and a rerun wrote."""
    rng = np.random.default_rng(0xC5)
    light = np.concatenate([short.cls["a23"], short.cls["a23"][:180]])
    gapped = np.concatenate([short.cls["b23"]] * 6 + [short.cls["b23"][:40]])
    idx = shuffled(rng, light, gapped)
    nq = len(idx)
    assert (len(light), len(gapped)) == (500, 1000)
    assert_overflows_both(short, light, nq)
    # every read the light pass finishes reserves once, room or not: the cursors stand at the sums when the arenas are grown; the rerun moves them on
    (li, ld), (gi, gd) = lengths(short.want, light), lengths(short.want, gapped)
    assert li + gi > grown_cap(initial_int_cap(nq), li) or ld + gd > grown_cap(initial_dbl_cap(nq), ld), "resize the case: the grown arenas hold the gapped pass's results"
    b, want = compose_batch(short.U, idx), compose_streams(short.want, idx)
    ctx = short.db.new_context()
    try:
        got, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        assert overflowed(passes, ["light", "gapped"])[0] == 0
        check_result(got, want, nq)
    finally:
        ctx.close()


def test_collapsed_copies(short, capfd, monkeypatch):
    """Case 6.  Case 1's batch three times over, collapsed: the representatives fill the arenas, the copies' slices come from the fan-out and the totals from the scan."""
    distinct = case1_indices(short)
    idx = shuffled(np.random.default_rng(0xC6), distinct, distinct, distinct)
    assert_overflows_both(short, distinct, len(idx))
    b, want, work = compose_batch(short.U, idx), compose_streams(short.want, idx), compose_streams(short.want, distinct)
    ctx = short.db.new_context()
    try:
        ctx.set_collapse(True)
        got, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
        assert passes[0].reads == len(distinct)
        assert overflowed(passes, ["light"]) == [0]
        assert got.extra[7] == got.copies == 2 * len(distinct)
        assert streams_equal(want, got), first_difference(want, got, len(idx))
        assert (len(got.ints), len(got.dbls)) == (int(want.int_off[-1]), int(want.dbl_off[-1]))
        assert [int(x) for x in got.counters[:8]] == expected_counters(work) and int(got.counters[8]) == work.alignments_out   # (the work done: the representatives')
    finally:
        ctx.close()


def test_memo_hits_already_in_the_arena(short, capfd, monkeypatch):
    """Case 7.  Fifty remembered queries are replayed into the arenas before the passes; the new reads then fill them, and growKeep moves the replayed slices."""
    first = np.concatenate([short.cls["c"][:25], short.cls["a23"][:25]])
    new = short.cls["a23"][25:315]
    idx = shuffled(np.random.default_rng(0xC7), first, new)
    fi, fd = lengths(short.want, first)
    assert fi <= initial_int_cap(len(first)) and fd <= initial_dbl_cap(len(first))
    ni, nd = lengths(short.want, new)
    assert ni > initial_int_cap(len(idx)) and nd > initial_dbl_cap(len(idx))   # (on top of the room the hits are given)
    ctx = short.db.new_context()
    try:
        ctx.set_memo(MEMO)
        got, passes, _ = run_traced(ctx, compose_batch(short.U, first), capfd, monkeypatch)
        overflowed(passes, [])
        check_result(got, compose_streams(short.want, first), len(first))
        got, passes, _ = run_traced(ctx, compose_batch(short.U, idx), capfd, monkeypatch)
        assert got.remembered == len(first) == 50 and got.copies == 0
        assert passes[0].reads == len(new)
        assert overflowed(passes, ["light"]) == [0]
        want, work = compose_streams(short.want, idx), compose_streams(short.want, new)
        assert streams_equal(want, got), first_difference(want, got, len(idx))
        assert [int(x) for x in got.counters[:8]] == expected_counters(work) and int(got.counters[8]) == work.alignments_out
    finally:
        ctx.close()


def test_wave_form_hands_over_to_the_lane_passes(short, capfd, monkeypatch):
    """Case 8.  The wave-per-read form has its own copy of the check (xm_wave_kernel.hip): a read that finds an arena full is left to the lane-per-read passes.
    Their first pass finds the cursors beyond the capacities, where the wave form left them, and the rerun has the room."""
    idx = case1_indices(short)
    assert_overflows_both(short, idx)
    b, want = compose_batch(short.U, idx), compose_streams(short.want, idx)
    ctx = short.db.new_context()
    try:
        got, passes, tiers = run_traced(ctx, b, capfd, monkeypatch, XM_WAVE="1")
        assert tiers and tiers[0][:2] == (0, len(idx)) and tiers[-1][2] > 0, tiers
        assert passes and passes[0].reads == tiers[-1][2], (tiers, passes)
        assert overflowed(passes, [passes[0].kind]) == [0]
        check_result(got, want, len(idx))
    finally:
        ctx.close()


# ---------------------------------------------------------------- the scan and the gather at their edges

EDGE_NQ = (1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192, 8193)   # 16 queries per thread, 256 threads per gather block, 4 096 queries per scan block


def edge_indices(s, nq, inverted):
    """The longest slices on the last query of every group of 16 (so of every block of 256 and of 4 096) and on the first of the next, slices without doubles
    everywhere else; `inverted`: the other way round.  Neighbouring long slices are different reads."""
    q = np.arange(nq)
    at_edge = (q % 16 == 15) | (q % 16 == 0)
    long_, none = s.cls["a23"], s.cls["d"]
    return np.where(at_edge != inverted, long_[q % len(long_)], none[q % len(none)])


@pytest.fixture(scope="module")
def warm(short):
    """One context for every edge case, its arenas grown by the largest batch of them all."""
    ctx = short.db.new_context()
    b = compose_batch(short.U, edge_indices(short, max(EDGE_NQ), True))
    ctx.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())
    yield ctx
    ctx.close()


def check_edges(s, ctx, idx, capfd, monkeypatch):
    b, want = compose_batch(s.U, idx), compose_streams(s.want, idx)
    got, passes, _ = run_traced(ctx, b, capfd, monkeypatch)
    assert passes
    overflowed(passes, [])
    assert np.array_equal(got.int_off, want.int_off) and np.array_equal(got.dbl_off, want.dbl_off)
    assert np.array_equal(got.ints, want.ints) and np.array_equal(np.asarray(got.dbls).view(np.int64), want.dbls.view(np.int64)), first_difference(want, got, len(idx))
    assert (len(got.ints), len(got.dbls)) == (int(got.int_off[-1]), int(got.dbl_off[-1]))   # (num_ints, num_dbls of the C result are the arrays' lengths)
    return got


@pytest.mark.parametrize("nq", EDGE_NQ)
def test_scan_and_gather_edges(short, warm, nq, capfd, monkeypatch):
    for inverted in (False, True):
        check_edges(short, warm, edge_indices(short, nq, inverted), capfd, monkeypatch)


def test_empty_double_stream(short, warm, capfd, monkeypatch):
    nq = 4097
    got = check_edges(short, warm, short.cls["d"][np.arange(nq) % len(short.cls["d"])], capfd, monkeypatch)
    assert len(got.dbls) == 0 and not np.any(got.dbl_off) and len(got.dbl_off) == nq + 1
    assert len(got.ints) == 2 * nq


def test_collapsed_totals_come_from_the_scan(short, capfd, monkeypatch):
    """4 097 queries drawn from 40 distinct ones (with pairs among them), collapsed: finishStreams takes its totals from the scan, not from the cursors."""
    rng = np.random.default_rng(0xED6)
    distinct = np.concatenate([short.cls["a23"][:14], short.cls["a5"][:8], short.cls["c"][:6], short.cls["d"][:8], short.cls["e"][:4]])
    assert len(distinct) == 40
    idx = np.concatenate([distinct, distinct[rng.integers(0, 40, 4097 - 40)]])[rng.permutation(4097)]
    ctx = short.db.new_context()
    try:
        ctx.set_collapse(True)
        got = check_edges(short, ctx, idx, capfd, monkeypatch)
        assert got.copies == 4097 - 40 and int(got.counters[0]) == 40
        work = compose_streams(short.want, distinct)
        assert [int(x) for x in got.counters[:8]] == expected_counters(work) and int(got.counters[8]) == work.alignments_out
    finally:
        ctx.close()
