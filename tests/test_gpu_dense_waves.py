"""Gapped passes of long reads in their dense shape on the GPU: several non-aligning 1 kb sections per wave, eight lanes per read, the rejection filter
(mapper_amd/csrc/xm_bound.h) on.  That is the regime in which a memory fault, a hang in a lane mask and a band that was too narrow all turned up while the filter
was built (profiles/r06/NOTES.md 2, 12, 15a), and the one in which each read of a wave works in its own region of the wave's LDS slot.  The other tests of the
tier reach it with one or two reads per wave only.

Shape.  The launch logic (xm_pass_plan.h, planLaunch, the gapped pass) gives a batch of long reads waveSlots = numCUs x 4 x XM_FULL_WAVES wave slots and
lpw = min(XM_FULL_LPW = 8, ceil(reads / waveSlots)) reads per wave, then - when the lanes would fill fewer waves than the GPU holds at a time - cuts lpw to
lanes / slotsHeld with slotsHeld = numCUs x 16 / contexts.  On an MI355X (256 CUs) with XM_FULL_WAVES=1 and FOUR contexts of the database open:
waveSlots = 1 024, lanes = 1 024 x 8 = 8 192 for a pass of >= 8 192 reads, slotsHeld = 4 096 / 4 = 1 024, and 8 192 / 8 = 1 024 waves is not fewer than that:
lpw stays 8.  A pass of R reads between 5 200 and 8 192 gets lanes = R and lpw = floor(R / 1 024) >= 5.  (One context: slotsHeld = 4 096 and lpw = 2.)
The shape is not assumed: every run reads the pass trace (XM_TRACE_PASSES=1, "[xm] pass N: gapped reads R ... lpw L waves W lanes/read G filter F" on fd 2)
and asserts, for the pass that ran the filter, L >= 5, R / W >= 5 and G = 8.  A change of the launch logic that loses the shape fails here.
(The arithmetic itself - xm_pass_plan.h, planLaunch - is pinned without a GPU for these cases in tests/test_pass_plan.py.)

What is compared: the oracle's streams bit for bit (with its observer of the filter's bound on: it raises when a search the bound rejects aligns), the
filter's counters against the observer's (tests/helpers.py filter_counters), and the work counters against the reference's minus what the filter skipped -
then the same batch in the other lane forms (XM_GROUP_SWEEP=0: eight lanes that each compute every cell; XM_GROUP_LANES=0: two lanes per read) and without the
filter."""
import os
import re
import numpy as np
import pytest

import oracle_lib as o
from helpers import streams_equal, first_difference, filter_counters, long_read_batch, filter_fuzz_case
from mapper_amd import api, synth

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count())   # (a command on the GPU box has 16 CPUs, whatever the machine reports)
CONTEXTS = 4
TRACE = re.compile(r"\[xm\] pass (\d+): gapped reads (\d+) scale \d+ lpw (\d+) waves (\d+) lanes/read (\d+) filter (\d)")


def run_dense(db, b, prm, capfd, monkeypatch, **env):
    """One call with the dense launch shape (the caller holds CONTEXTS contexts of the database) -> (result, [(reads, lpw, waves, lanes per read, filter)] of its gapped passes)."""
    monkeypatch.setenv("XM_TRACE_PASSES", "1")
    monkeypatch.setenv("XM_FULL_WAVES", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    try:
        got = db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters(**prm))
    finally:
        err = capfd.readouterr().err
        for k in env:
            monkeypatch.delenv(k)
    return got, [tuple(int(x) for x in m.groups()[1:]) for m in TRACE.finditer(err)]


def assert_dense(passes, filter_on=True, lanes_per_read=8):
    """The widest gapped pass (the one that holds the batch; reruns of a few reads may follow) ran several reads per wave, with the filter as asked."""
    assert passes, "no gapped pass in the trace"
    reads, lpw, waves, lpr, filt = max(passes)
    assert filt == (1 if filter_on else 0), passes
    assert lpw >= 5 and reads / waves >= 5, ("fewer than five reads per wave", passes)
    assert lpr == lanes_per_read, passes


def work_counters(got, want, filter_ran):
    """counters[:8] against the oracle's, PathAligner calls and nodes without what the filter skipped (as test_grch38_regime_alignments_equal_oracle compares them)"""
    wc = [int(x) for x in want.counters[:9]]
    skipped_calls = int(want.counters[16]) if filter_ran else 0
    skipped = int(want.counters[12]) + int(want.counters[17]) if filter_ran else 0
    return [int(x) for x in got.counters[:8]] == [wc[0], wc[1] + wc[2], wc[2], wc[3], wc[5], wc[6] - skipped_calls, wc[7] - skipped, wc[8]]


def check_forms(db, b, want, prm, capfd, monkeypatch):
    """The batch in its dense shape in every lane form, against the oracle's run (want, with the observer on)."""
    got, passes = run_dense(db, b, prm, capfd, monkeypatch)
    assert_dense(passes)
    assert streams_equal(want, got), first_difference(want, got, b.nq)
    assert got.extra[3] == 1
    ok, what = filter_counters(got.counters, got.extra, want.counters)
    assert ok, what
    assert work_counters(got, want, True)
    for knob, lanes in (("XM_GROUP_SWEEP", 8), ("XM_GROUP_LANES", 2)):
        alt, passes = run_dense(db, b, prm, capfd, monkeypatch, **{knob: "0"})
        assert_dense(passes, lanes_per_read=lanes)
        assert streams_equal(want, alt), (knob, first_difference(want, alt, b.nq))
        ok, what_alt = filter_counters(alt.counters, alt.extra, want.counters)
        assert ok, (knob, what_alt)
        assert work_counters(alt, want, True), knob
    off, passes = run_dense(db, b, prm, capfd, monkeypatch, XM_BOUND_FILTER="0")
    assert_dense(passes, filter_on=False, lanes_per_read=2)   # (eight lanes per read only where the filter runs: its recurrence is what uses them)
    assert streams_equal(want, off), ("XM_BOUND_FILTER=0", first_difference(want, off, b.nq))
    assert off.extra[3] == 0 and off.extra[1] == 0 and off.extra[5] == 0
    assert off.counters[5] == want.counters[6] and off.counters[6] == want.counters[7] and work_counters(off, want, False)
    return what


class Contexts:
    """CONTEXTS contexts of one database (the first is the database itself): the extra ones only divide the wave slots the launch logic counts on."""

    def __init__(self, contigs, **kw):
        self.db = api.ReferenceDatabase(contigs, **kw)
        self.extra = [self.db.new_context() for _ in range(CONTEXTS - 1)]

    def __enter__(self):
        return self.db

    def __exit__(self, *a):
        for c in self.extra:
            c.close()
        self.db.close()


def test_dense_waves_configs4_as_stated(capfd, monkeypatch):
    """configs[4] as stated (5 % substitutions + 5 % indel events: almost no section aligns, most pieces and searches are proved unalignable), 2 000 reads of
    10 kb = 20 000 sections on the 2 Mb synthetic reference: one gapped pass of 20 000 reads, lpw 8 on 1 024 waves."""
    ref = synth.synthetic_reference(2_000_000, seed=0xEC011)
    b = long_read_batch(ref, 2000, 0.05, 0.05, seed=0xDE05)
    with o.observe_bound():
        want = o.OracleReference([("r", ref)]).align(b, o.make_params(), threads=THREADS)
    with Contexts([("r", ref)], max_query_length=1000) as db:
        what = check_forms(db, b, want, {}, capfd, monkeypatch)
    assert what["oracle_observer"]["pieces_rejected"] > 0.5 * what["oracle_observer"]["pieces_examined"] > 0, what


def test_dense_waves_milder_errors(capfd, monkeypatch):
    """Milder errors (2 % + 0.2 %: most sections align, searches that find their answer), 820 reads = 8 200 sections on the 2 Mb synthetic reference: lpw 8 on
    1 024 waves (>= 8 192 reads).  (The GRCh38-shaped reference with minInterestingSize = 13 costs the oracle ~0.1 s per section and thread - minutes for a batch
    this size - so the dense shape is tested on the synthetic one; test_grch38_regime_alignments_equal_oracle has the minIS = 13 walk with the filter.)"""
    ref = synth.synthetic_reference(2_000_000, seed=0xEC011)
    b = long_read_batch(ref, 820, 0.02, 0.002, seed=0xDE07)
    with o.observe_bound():
        want = o.OracleReference([("r", ref)]).align(b, o.make_params(), threads=THREADS)
    with Contexts([("r", ref)], max_query_length=1000) as db:
        check_forms(db, b, want, {}, capfd, monkeypatch)


@pytest.mark.parametrize("case", range(4))
def test_dense_waves_filter_fuzz(case, capfd, monkeypatch):
    """scripts/cpu_filter_fuzz.py's generator (tests/helpers.py filter_fuzz_case: lengths 330-1500, five error regimes, N bases, a repeated stretch, prices off the
    grid) at a fixed seed, 6 600 - 7 400 reads per batch (at least 5 x 1 024 must reach the gapped pass for lpw >= 5: smaller batches than the script's 3-9 k
    would test two to four reads per wave).  Streams and counters as above, in the product's lane form."""
    rng = np.random.default_rng(0xF0 + case)
    ref, prm, b = filter_fuzz_case(rng, 6600, 7400)
    p = o.make_params(prm)
    with o.observe_bound():
        want = o.OracleReference([("r", ref)]).align(b, p, threads=THREADS)
    with Contexts([("r", ref)], max_query_length=1500) as db:
        got, passes = run_dense(db, b, prm, capfd, monkeypatch)
    assert_dense(passes)
    assert streams_equal(want, got), (case, first_difference(want, got, b.nq))
    ok, what = filter_counters(got.counters, got.extra, want.counters)
    assert got.extra[3] == 1 and ok, (case, what)
    assert work_counters(got, want, True), case
