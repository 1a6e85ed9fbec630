"""The host's confidence table (mapper_amd/csrc/xm_conf_table.h: ConfTable) without a GPU, through the host simulation library.  The table decides outputs:
quicklyConfidentInBestAlignment takes its pow / log term from it, so an entry that cannot be found again, or one with another value than
confidenceLengthOnHost gives, changes alignments.  Here the insert half (ConfTable) and the lookup half (confLookup of xm_defs.h, what the kernels run) are
held against each other, and the reset rules and the seeding policy of ConfTable::prepare are pinned: running sums 0, m, m + m, ... per query length, at most
min(4096, floor(limit / m) + 2) of them with limit = length * MaxErrorRate + Max_PenaltySpan + m, cut at the first sum above limit; a length whose steps
exceed what is left of the call's budget is skipped and not marked as seeded."""
import math

import numpy as np

import hostsim_lib as hs
import oracle_lib

GRANULARITY = 8.0
TOTAL = 2 * 4_600_000


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def seed_sums(params, length):
    """-> (steps the length costs the budget, the sums that are seeded), by the rule in the module docstring"""
    m = params.MutationPenalty
    limit = length * params.MaxErrorRate + params.Max_PenaltySpan + m
    steps = min(4096, math.floor(limit / m) + 2)
    sums, pen = [], 0.0
    for _ in range(steps):
        if pen > limit:
            break
        sums.append(pen)
        pen += m
    return steps, sums


def key_set(penalties, lens):
    return set(zip(bits(penalties).tolist(), np.asarray(lens).tolist()))


def seeded_keys(params, lengths):
    return {(int(bits([s])[0]), n) for n in lengths for s in seed_sums(params, n)[1]}


def table_keys(t):
    pen, ln, val = t.entries()
    return key_set(pen, ln)


def test_every_inserted_key_is_found_again_through_two_growths():
    params = oracle_lib.make_params(MutationPenalty=0.3)
    t = hs.SimConfTable()
    t.prepare(params, [], GRANULARITY, TOTAL, 0)
    assert t.state()[:2] == (1 << 14, 0)
    rng = np.random.default_rng(0xC0F1)
    pen, ln = [], []
    for length in range(40, 2040, 100):   # 20 lengths x 500 running sums of a penalty that is no dyadic fraction
        s = 0.0
        for _ in range(500):
            pen.append(s)
            ln.append(length)
            s += 0.3
    pen += rng.uniform(0.0, 60.0, 10_000).tolist()   # arbitrary doubles
    ln += rng.integers(20, 5000, 10_000).tolist()
    pen, ln = np.array(pen), np.array(ln, dtype=np.int32)
    assert len(key_set(pen, ln)) == 20_000
    order = rng.permutation(20_000)   # the two kinds mixed
    pen, ln = pen[order], ln[order]
    sizes = set()
    for at in range(0, 20_000, 250):
        assert t.insert(pen[at:at + 250], ln[at:at + 250]).all()
        slots, entries, dirty = t.state()
        assert entries == at + 250 and dirty
        assert slots & (slots - 1) == 0 and entries * 2 <= slots   # a power of two, at most half full
        sizes.add(slots)
    assert sorted(sizes) == [1 << 14, 1 << 15, 1 << 16]
    found, values = t.lookup(pen, ln)
    assert found.all()
    assert np.array_equal(bits(values), bits(hs.conf_values(pen, ln, params, GRANULARITY, TOTAL)))
    # never inserted: known penalties under other lengths, known lengths under other penalties
    miss_pen = np.concatenate([pen[:500], rng.uniform(60.0, 90.0, 500)])
    miss_len = np.concatenate([ln[:500] + 10_000, ln[500:1000]])
    assert not (key_set(miss_pen, miss_len) & key_set(pen, ln))
    found, _ = t.lookup(miss_pen, miss_len)
    assert not found.any()
    assert t.state()[1] == 20_000


def test_duplicate_insert_changes_nothing_and_upload_mark_clears_dirty():
    t = hs.SimConfTable()
    t.prepare(oracle_lib.make_params(), [], GRANULARITY, TOTAL, 0)
    assert t.state() == (1 << 14, 0, True)   # (a fresh table has not been uploaded yet)
    t.mark_uploaded()
    assert t.state()[2] is False
    assert t.insert([2.5], [100]).tolist() == [True]
    assert t.state() == (1 << 14, 1, True)
    t.mark_uploaded()
    assert t.state() == (1 << 14, 1, False)
    assert t.insert([2.5], [100]).tolist() == [False]
    assert t.state() == (1 << 14, 1, False)
    assert t.insert([2.5, 2.5], [101, 100]).tolist() == [True, False]   # same penalty, another length: another key
    assert t.state() == (1 << 14, 2, True)


def test_seeding_puts_exactly_the_running_sums_within_the_limit():
    for params, lengths in ((oracle_lib.make_params(), (36, 150, 301)), (oracle_lib.make_params(MutationPenalty=0.3), (36, 150, 301)),
                            (oracle_lib.make_params(MutationPenalty=0.3), (60_000,))):   # (the last: the cap of 4096 steps)
        t = hs.SimConfTable()
        t.prepare(params, lengths, GRANULARITY, TOTAL, 1 << 18)
        want = seeded_keys(params, lengths)
        assert table_keys(t) == want
        for n in lengths:
            steps, sums = seed_sums(params, n)
            limit = n * params.MaxErrorRate + params.Max_PenaltySpan + params.MutationPenalty
            assert 0 < len(sums) <= steps and all(s <= limit for s in sums)
        assert t.state()[1] == len(want) == sum(len(seed_sums(params, n)[1]) for n in lengths)
        pen, ln, val = t.entries()
        assert np.array_equal(bits(val), bits(hs.conf_values(pen, ln, params, GRANULARITY, TOTAL)))
    assert len(seed_sums(oracle_lib.make_params(), 36)[1]) == 6       # limit 5.1: 0 .. 5
    assert len(seed_sums(oracle_lib.make_params(MutationPenalty=0.3), 60_000)[1]) == 4096


def test_seed_budget_skips_what_does_not_fit_and_later_calls_catch_up():
    params = oracle_lib.make_params()
    t = hs.SimConfTable()
    lengths = [36, 700, 650, 600, 550, 150, 500, 301, 100]
    t.prepare(params, lengths, GRANULARITY, TOTAL, 0)
    assert t.state()[1] == 0
    # steps 7, 73, 68, 63, 58, 18 leave 13 of 300: 500 (53 steps) and 301 (33) do not fit, 100 (13) behind them does
    assert [seed_sums(params, n)[0] for n in lengths] == [7, 73, 68, 63, 58, 18, 53, 33, 13]
    t.prepare(params, lengths, GRANULARITY, TOTAL, 300)
    first = [36, 700, 650, 600, 550, 150, 100]
    assert table_keys(t) == seeded_keys(params, first)
    found, _ = t.lookup([0.0, 0.0, 0.0], [500, 301, 100])
    assert found.tolist() == [False, False, True]
    t.prepare(params, lengths, GRANULARITY, TOTAL, 300)   # room left: the skipped lengths
    assert table_keys(t) == seeded_keys(params, lengths)
    t.mark_uploaded()
    t.prepare(params, lengths, GRANULARITY, TOTAL, 300)   # every length is seeded: nothing to do
    assert table_keys(t) == seeded_keys(params, lengths) and t.state()[2] is False


def test_settings_that_change_the_values_empty_the_table_and_the_error_rate_seeds_again():
    base = dict(MutationPenalty=1.0, Max_PenaltySpan=0.5, MaxErrorRate=0.1)
    lengths = (36, 150, 301)

    def seeded():
        t = hs.SimConfTable()
        t.prepare(oracle_lib.make_params(**base), lengths, GRANULARITY, TOTAL, 1 << 18)
        assert t.insert([1.7], [150]).all()   # (a key that came in through the miss path)
        t.mark_uploaded()
        return t, t.state()[1]

    for change, granularity, total in ((dict(Max_PenaltySpan=0.75), GRANULARITY, TOTAL), (dict(MutationPenalty=0.3), GRANULARITY, TOTAL), ({}, GRANULARITY * 2, TOTAL),
                                       ({}, GRANULARITY, TOTAL + 2)):
        t, n = seeded()
        assert n == len(seeded_keys(oracle_lib.make_params(**base), lengths)) + 1
        params = oracle_lib.make_params(**dict(base, **change))
        t.prepare(params, lengths, granularity, total, 0)
        assert t.state() == (1 << 14, 0, True)
        t.prepare(params, lengths, granularity, total, 1 << 18)   # (and it is seeded for the new settings, with their values)
        assert table_keys(t) == seeded_keys(params, lengths)
        pen, ln, val = t.entries()
        assert np.array_equal(bits(val), bits(hs.conf_values(pen, ln, params, granularity, total)))
    t, n = seeded()
    before = t.entries()
    t.prepare(oracle_lib.make_params(**base), lengths, GRANULARITY, TOTAL, 1 << 18)   # nothing changed: nothing happens
    assert t.state() == (1 << 14, n, False)
    wider = oracle_lib.make_params(**dict(base, MaxErrorRate=0.2))
    t.prepare(wider, lengths, GRANULARITY, TOTAL, 1 << 18)
    assert table_keys(t) == key_set(before[0], before[1]) | seeded_keys(wider, lengths)
    assert t.state()[1] > n and t.state()[2] is True
    found, values = t.lookup(before[0], before[1])
    assert found.all() and np.array_equal(bits(values), bits(before[2]))
