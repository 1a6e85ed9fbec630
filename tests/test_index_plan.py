"""The planner of an index build (mapper_amd/csrc/xm_index_plan.h: tableShape, planGroups, layoutGroup, sortKeyBits) without a GPU, through the host
simulation library.  It is the arithmetic the host builder (HostIndex::hashLengths) and the GPU builder (deviceHashLengths) share, so that their tables
agree by construction; the GPU builder runs it between its launches.  Every check is against a plain restatement written here."""
import numpy as np

import hostsim_lib as hs

INT32_MAX = 2 ** 31 - 1


def test_table_shape_limits():
    """Per-key limit max(L * L, maxNumShortMatches) in [1, 32 766] (M/HashBlock_Database.java:569-576); capacity in [1, INT32_MAX / 2] (M/PackedMap.java:22-25)."""
    for L, want in ((1, 5), (2, 5), (3, 9), (181, 32761), (182, 32766), (30000, 32766)):
        assert hs.table_shape(1001, L, 5) == (1001, want), L
    for cap in (0, -1, -INT32_MAX):
        assert hs.table_shape(cap, 20, 5)[0] == 1
    assert hs.table_shape(INT32_MAX, 20, 5)[0] == INT32_MAX // 2
    assert hs.table_shape(INT32_MAX // 2, 20, 5)[0] == INT32_MAX // 2 and hs.table_shape(INT32_MAX // 2 + 1, 20, 5)[0] == INT32_MAX // 2
    assert hs.table_shape(7, 1, 0) == (7, 1) and hs.table_shape(7, 1, -3) == (7, 1)   # (never below 1)


def test_plan_groups_fixed_histograms():
    hist = [0, 0, 7, 3, 0, 9, 1]
    assert hs.plan_groups(hist, 0, 1000) == [(0, 6, 20)]
    assert hs.plan_groups(hist, 0, 20) == [(0, 6, 20)]
    assert hs.plan_groups(hist, 2, 1000) == [(2, 6, 20)]
    # budget 10: tables 0..3 fill it exactly and the empty table 4 still joins them (the sum stays within the budget), then 9 + 1 fill the second group exactly
    assert hs.plan_groups(hist, 0, 10) == [(0, 4, 10), (5, 6, 10)]
    assert hs.plan_groups([0, 0, 7, 3, 1, 9, 1], 0, 10) == [(0, 3, 10), (4, 5, 10), (6, 6, 1)]
    assert hs.plan_groups(hist, 0, 9) == [(0, 2, 7), (3, 4, 3), (5, 5, 9), (6, 6, 1)]
    # a table that alone exceeds the budget is a group on its own: its neighbours are not pulled into it
    assert hs.plan_groups([4, 50, 4], 0, 10) == [(0, 0, 4), (1, 1, 50), (2, 2, 4)]
    assert hs.plan_groups([50, 4, 4, 4], 0, 10) == [(0, 0, 50), (1, 2, 8), (3, 3, 4)]
    # budget 1: runs of empty tables join, every non-empty table stands alone or behind the empty ones before it
    assert hs.plan_groups([0, 0, 1, 0, 3, 1, 0, 0], 0, 1) == [(0, 3, 1), (4, 4, 3), (5, 7, 1)]
    assert hs.plan_groups([2, 0, 0, 2], 0, 1) == [(0, 0, 2), (1, 2, 0), (3, 3, 2)]
    assert hs.plan_groups([0, 0, 0], 0, 1) == [(0, 2, 0)]
    assert hs.plan_groups([3], 0, 1) == [(0, 0, 3)]


def test_plan_groups_sweep():
    """Seeded histograms (all-zero ones among them) and budgets: the groups are consecutive and cover [minLen, maxLen] once, carry the sum of their tables, exceed
    the budget only as a single table, and none could have taken the next table."""
    rng = np.random.default_rng(0x1D8)
    for it in range(400):
        n = int(rng.integers(1, 40))
        kind = it % 4
        if kind == 0:
            hist = np.zeros(n, dtype=np.int64)
        elif kind == 1:
            hist = rng.integers(0, 3, size=n)
        else:
            hist = rng.integers(0, 1000, size=n) * (rng.random(n) < 0.6)
        hist = [int(v) for v in hist]
        min_len = int(rng.integers(0, n))
        budget = int(rng.choice([1, 2, 10, 500, 1000, 5000, 10 ** 9]))
        groups = hs.plan_groups(hist, min_len, budget)
        assert groups[0][0] == min_len and groups[-1][1] == n - 1, (hist, min_len, budget)
        for i, (lo, hi, recs) in enumerate(groups):
            assert lo <= hi and recs == sum(hist[lo:hi + 1]), (hist, min_len, budget)
            assert recs <= budget or lo == hi, (hist, min_len, budget)
            if i + 1 < len(groups):
                assert groups[i + 1][0] == hi + 1 and recs + hist[hi + 1] > budget, (hist, min_len, budget)


def test_layout_group():
    """A group's tables side by side, capacity + 1 offset entries each; a table without records is the (1, 1) placeholder whatever its planned capacity."""
    hist = [0, 5, 0, 12, 1, 0]
    cap = [0, 11, 13, 17, 19, 23]      # (table 0 lies below minInterestingSize: no planned shape)
    mx = [0, 5, 9, 16, 25, 36]
    tables, n_entries = hs.layout_group(hist, cap, mx, 0, 5)
    want_shape = [(1, 1), (11, 5), (1, 1), (17, 16), (19, 25), (1, 1)]
    assert [(c, m) for _, c, m in tables] == want_shape
    base = 0
    for (b, c, _) in tables:
        assert b == base
        base += c + 1
    assert n_entries == base == sum(c + 1 for c, _ in want_shape)
    tables, n_entries = hs.layout_group(hist[:5], cap[:5], mx[:5], 3, 4)   # a group in the middle: its bases start at 0
    assert tables == [(0, 17, 16), (18, 19, 25)] and n_entries == 38
    tables, n_entries = hs.layout_group([0, 0], [INT32_MAX // 2, 7], [5, 5], 0, 1)
    assert tables == [(0, 1, 1), (2, 1, 1)] and n_entries == 4
    tables, n_entries = hs.layout_group([1, 1], [INT32_MAX // 2, INT32_MAX // 2], [5, 5], 0, 1)   # (64-bit bases)
    assert tables == [(0, INT32_MAX // 2, 5), (INT32_MAX // 2 + 1, INT32_MAX // 2, 5)] and n_entries == 2 * (INT32_MAX // 2 + 1)


def test_sort_key_bits():
    """tableBits: the smallest b >= 1 with 2^b >= nTables; posBits: the smallest b >= 1 with last >> b == 0, one more with the multi flag in bit 0."""
    for n_tables, want in ((1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (151, 8)):
        assert hs.sort_key_bits(1000, False, n_tables)[1] == want, n_tables
    for last, want in ((1, 1), (2 ** 31 - 1, 31), (2 ** 32, 33), (2 ** 35, 36)):
        assert want == max(1, last.bit_length())
        assert hs.sort_key_bits(last, False, 7) == (want, 3), last
        assert hs.sort_key_bits(last, True, 7) == (want + 1, 3), last
    assert hs.sort_key_bits(0, False, 1) == (1, 1)
