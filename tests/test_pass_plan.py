"""The pass planner of an align call (mapper_amd/csrc/xm_pass_plan.h: PassKnobs, BatchPolicy, planLaunch, nextPass) without a GPU, through the host
simulation library.  It is the code the product runs between its launches - plain C++ with no device input but the CU count - so the launch shapes that
tests/test_gpu_dense_waves.py and tests/test_gpu_parity.py::test_long_reads_sharing_waves_on_gpu read back from the pass trace on a GPU are pinned here as
well, with what DESIGN.md 4c states and with invariants of the scratch layout over a seeded sweep.

The scratch budget is a target, not a bound: the caller's allocation may fail, and it then plans again with half of it.  What the arithmetic guarantees
is that a plan overshoots the budget by no more than the rounding to whole blocks of four waves of 64 lanes (a light-pass lane is its arena and its region)
plus, in the light pass, the one gapped-pass lane (or plain arena of the gapped scale) the scratch always keeps room for, plus 1 KiB."""
import numpy as np
import pytest

import hostsim_lib as hs

CUS = 256
GIB = 1 << 30
AMPLE = 4096 * GIB   # (the arithmetic takes any budget; no such GPU)
KNOBS = ("XM_GAPPED_SCALE", "XM_GAPPED_FACTOR", "XM_ARENA_KB", "XM_SCRATCH_GIB", "XM_LIGHT_WAVES", "XM_FULL_WAVES", "XM_FULL_LPW", "XM_LIGHT_LPW", "XM_LIGHT_LEVEL", "XM_HEAVY_HINT",
         "XM_TAPER_PCT", "XM_PAIR_LANES", "XM_GROUP_LANES", "XM_BOUND_FILTER", "XM_SEARCH_POOL", "XM_GAPPED_TMP_PCT", "XM_LIGHT_TMP_KB", "XM_REGION_KB", "XM_HANDOVER", "XM_WAVE",
         "XM_GROUP_SWEEP", "XM_TRACE_PASSES", "XM_PROF_GAPPED_ONLY")


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def light_then_gapped(n_reads, n_heavy, longest_mate, contexts=1, budget=AMPLE, cus=CUS, paired=False):
    """The first two launches of a call as alignResidentLocked runs them: the light pass over the batch, then the gapped pass over n_heavy of its reads in the
    scratch the light pass's plan sized -> (light plan, gapped plan, the gapped pass's state)."""
    kw = dict(longest_mate=longest_mate, paired=paired, contexts=contexts)
    _, st = hs.pass_policy(**kw)
    light = hs.plan_launch(st, n_reads, n_reads, cus, budget, 0, **kw)
    st["nRegions"], st["regionsTotal"] = light["nRegions"], light["regionsTotal"]
    kind, n, _, _, st = hs.next_pass(st, {"nHeavy": n_heavy}, **kw)
    assert (kind, n) == ("gapped", n_heavy)
    return light, hs.plan_launch(st, n_heavy, n_reads, cus, budget, light["scratchBytes"], **kw), st


def test_batch_policy_sizes():
    """Seed scale 1 up to 320 bases, 4 up to 1 280, 16 beyond; the gapped pass at 4, 16, 64; arena 288 KiB, light temporaries 48 KiB, region 72 KiB (single reads)
    or 120 KiB (pairs) x the seed scale + the saved context; the gapped pass's temporaries a fifth of 7/12 of its arena for short reads (search pool on), all
    of it + the long chain's arrays for long reads (filter allowed, no pool); the expensive-first order for single short reads only."""
    saved = None
    for mate, seed in ((36, 1), (320, 1), (321, 4), (1280, 4), (1281, 16), (30000, 16)):
        for paired in (False, True):
            pol, st = hs.pass_policy(mate, paired)
            assert (pol["seedScale"], pol["gappedScale"], pol["longReads"]) == (seed, 4 * seed, int(seed > 1))
            assert pol["arenaUnit"] == 288 * 1024 and pol["lightTmpUnit"] == 48 * 1024
            extra = pol["regionBytes"] - (120 if paired else 72) * 1024 * seed
            saved = extra if saved is None else saved
            assert extra == saved and 0 < extra < 64 * 1024 and extra % 16 == 0
            arena = 288 * 1024 * 4 * seed
            whole = arena - ((arena * 5 // 12) & ~15)
            if seed == 1:
                assert pol["gappedTmpBytes"] == (whole // 5) & ~15
            else:
                assert pol["gappedTmpBytes"] >= whole & ~15 and (pol["gappedTmpBytes"] - (whole & ~15)) % 4096 == 0
            assert (pol["boundFilterOn"], pol["searchPoolOn"]) == (int(seed > 1), int(seed == 1))
            assert pol["heavyHint"] == (64 if seed == 1 and not paired else 0)
            assert pol["scratchWanted"] == 200 * GIB
            assert (st["heavy"], st["hoMode"], st["scale"], st["overflowScale"], st["regionsTotal"]) == (0, 1, seed, seed, 0)
    assert hs.pass_policy(150, context_scratch=8 * GIB)[0]["scratchWanted"] == 8 * GIB


def test_wave_budget_follows_the_contexts_of_the_gpu():
    """alone 8 / 4 waves per SIMD worth of light / gapped lanes, two contexts 6 / 3 each, three 4 / 2; long reads 2 / 8 whatever the contexts."""
    for contexts, want in ((1, (8, 4)), (2, (6, 3)), (3, (4, 2)), (4, (3, 1)), (12, (2, 1))):
        pol, _ = hs.pass_policy(150, contexts=contexts)
        assert (pol["lightWaves"], pol["fullWaves"]) == want and (pol["lightLpw"], pol["fullLpw"]) == (64, 32)
        pol, _ = hs.pass_policy(1000, contexts=contexts)
        assert (pol["lightWaves"], pol["fullWaves"]) == (2, 8) and (pol["lightLpw"], pol["fullLpw"]) == (64, 8)


def test_design_4c_shapes():
    """DESIGN.md 4c on 256 CUs, one context, ample scratch."""
    light, gapped, _ = light_then_gapped(1_000_000, 200_000, 150)
    assert (light["lpw"], light["nWaves"], light["block"], light["boundFilter"], light["pairLanes"], light["poolBuffers"]) == (64, CUS * 4 * 8, 256, 0, 0, 0)
    assert (gapped["lpw"], gapped["nWaves"], 1 << gapped["pairLanes"], gapped["boundFilter"]) == (32, CUS * 4 * 4, 2, 0)
    assert gapped["poolBuffers"] == gapped["nWaves"] and gapped["firstStride"] == gapped["nWaves"] and gapped["firstItem"] == 32 * gapped["nWaves"]   # (expensive-looking reads first)
    assert gapped["scratchBytes"] == 0   # (saved regions alive: the light pass sized the scratch)
    light, gapped, _ = light_then_gapped(1_000_000, 200_000, 150, paired=True)
    assert (gapped["lpw"], gapped["nWaves"], 1 << gapped["pairLanes"], gapped["firstStride"]) == (32, CUS * 4 * 4, 2, 0)   # (pairs: list order)
    light, gapped, st = light_then_gapped(100_000, 100_000, 1000)
    assert (light["lpw"], light["nWaves"], light["grid"]) == (64, 1563, 391)   # (100 000 reads do not fill the 2 waves per SIMD worth of light lanes)
    assert (st["scale"], gapped["lpw"], gapped["nWaves"], 1 << gapped["pairLanes"], gapped["boundFilter"], gapped["boundFilterArg"], gapped["poolBuffers"]) == (16, 8, CUS * 4 * 8, 8, 1, 3, 0)


def test_shapes_the_gpu_tests_read_from_the_trace(monkeypatch):
    """tests/test_gpu_dense_waves.py and test_long_reads_sharing_waves_on_gpu: 1 kb reads, XM_FULL_WAVES=1, 256 CUs."""
    monkeypatch.setenv("XM_FULL_WAVES", "1")
    _, g, _ = light_then_gapped(9000, 9000, 1000)
    assert (g["lpw"], g["nWaves"], g["grid"], g["block"], g["boundFilter"], 1 << g["pairLanes"]) == (2, 4096, 1024, 256, 1, 8)
    for reads in (8192, 9000, 20000):
        _, g, _ = light_then_gapped(reads, reads, 1000, contexts=4)
        assert (g["lpw"], g["nWaves"], g["boundFilter"], 1 << g["pairLanes"]) == (8, 1024, 1, 8), reads
    _, g, _ = light_then_gapped(7400, 6000, 1000, contexts=4)
    assert (g["lpw"], g["nWaves"]) == (5, 1200)
    monkeypatch.setenv("XM_GROUP_LANES", "0")
    assert light_then_gapped(20000, 20000, 1000, contexts=4)[1]["pairLanes"] == 1
    monkeypatch.delenv("XM_GROUP_LANES")
    monkeypatch.setenv("XM_GROUP_SWEEP", "0")
    g = light_then_gapped(20000, 20000, 1000, contexts=4)[1]
    assert (g["pairLanes"], g["boundFilterArg"]) == (3, 1)
    monkeypatch.delenv("XM_GROUP_SWEEP")
    monkeypatch.setenv("XM_BOUND_FILTER", "0")
    g = light_then_gapped(20000, 20000, 1000, contexts=4)[1]
    assert (g["lpw"], g["pairLanes"], g["boundFilter"], g["boundFilterArg"]) == (8, 1, 0, 0)   # (eight lanes per read only where the filter runs)


def check_plan(pl, st, pol, n_todo, budget, held):
    assert 1 <= pl["lpw"] <= 64 and pl["block"] in (64, 128, 192, 256) and pl["grid"] >= 1
    assert pl["lanes"] == pl["grid"] * (pl["block"] // 64) * pl["lpw"]
    assert 0 <= pl["grid"] * (pl["block"] // 64) - pl["nWaves"] < 4   # (whole blocks of four waves)
    assert not pl["boundFilter"] or (pl["lpw"] <= 8 and st["heavy"] and pol["boundFilterOn"] and st["scale"] >= 16)
    assert pl["pairLanes"] in (0, 1, 3) and (pl["pairLanes"] != 3 or pl["boundFilter"]) and (pl["pairLanes"] == 0 or (st["heavy"] and pl["lpw"] <= 32))
    assert pl["firstItem"] <= n_todo
    need = pl["regionsTotal"] + pl["lanes"] * pl["arenaBytes"]
    rounding = 256 * (pl["arenaBytes"] + (pol["regionBytes"] if st["hoMode"] == 1 else 0))
    if st["hoMode"] != 1 and st["regionsTotal"] > 0:   # saved regions alive: the scratch stays where it is, and the launch fits behind the pool
        assert pl["scratchBytes"] == 0 and pl["regionsTotal"] == st["regionsTotal"] and need <= held
    elif st["hoMode"] == 1:
        gapped_arena = pol["arenaUnit"] * pol["gappedScale"]
        gapped_lane = pol["regionBytes"] + pol["gappedTmpBytes"]
        assert pl["nRegions"] >= pl["lanes"] and pl["regionsTotal"] == pl["nRegions"] * pol["regionBytes"]
        assert pl["gappedReserve"] >= max(gapped_lane, gapped_arena)
        assert max(need, pl["regionsTotal"] + pl["gappedReserve"]) <= pl["scratchBytes"] <= budget + rounding + max(gapped_lane, gapped_arena) + 1024
    else:
        assert pl["regionsTotal"] == 0 and need == pl["scratchBytes"] <= budget + rounding


def test_plan_invariants_over_a_sweep(monkeypatch):
    rng = np.random.default_rng(0x9A55)
    ranges = {"XM_LIGHT_WAVES": (1, 16), "XM_FULL_WAVES": (1, 16), "XM_FULL_LPW": (1, 64), "XM_LIGHT_LPW": (1, 64), "XM_ARENA_KB": (64, 2048), "XM_LIGHT_TMP_KB": (16, 512),
              "XM_REGION_KB": (32, 512), "XM_GAPPED_TMP_PCT": (5, 100), "XM_HEAVY_HINT": (0, 200), "XM_PAIR_LANES": (0, 1), "XM_GROUP_LANES": (0, 1), "XM_BOUND_FILTER": (0, 1),
              "XM_SEARCH_POOL": (0, 1), "XM_HANDOVER": (0, 1)}
    planned = {"light": 0, "gapped": 0, "behind_pool": 0, "rerun": 0}
    for it in range(400):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k in rng.choice(sorted(ranges), size=int(rng.integers(0, 5)), replace=False):
            monkeypatch.setenv(k, str(int(rng.integers(ranges[k][0], ranges[k][1] + 1))))
        if rng.integers(0, 4) == 0:
            monkeypatch.setenv("XM_GAPPED_SCALE", str(1 << int(rng.integers(0, 5))))
        kw = dict(longest_mate=int(rng.choice([100, 250, 320, 321, 1000, 1280, 5000])), paired=bool(rng.integers(0, 2)), contexts=int(rng.integers(1, 6)))
        cus = int(rng.choice([8, 64, 228, 256, 304]))
        budget = int(rng.choice([64 << 20, GIB, 8 * GIB, 150 * GIB, AMPLE])) + int(rng.integers(0, 1 << 20))
        nq = int(rng.choice([1, 3, 200, 5000, 9000, 100_000, 1_000_000, 3_000_000]))
        pol, st = hs.pass_policy(**kw)
        n_todo, held = nq, 0
        for launch in range(6):   # a call: light pass, gapped pass, reruns, with the lists a random part of what ran
            pl = hs.plan_launch(st, n_todo, nq, cus, budget, held, **kw)
            check_plan(pl, st, pol, n_todo, budget, held)
            planned["light" if not st["heavy"] else ("behind_pool" if st["regionsTotal"] else ("gapped" if st["scale"] == pol["gappedScale"] else "rerun"))] += 1
            held = max(held, pl["scratchBytes"])
            st["nRegions"], st["regionsTotal"] = pl["nRegions"], pl["regionsTotal"]
            part = lambda: int(rng.integers(0, n_todo + 1)) if rng.integers(0, 2) else 0
            ctl = {"nHeavy": part() if not st["heavy"] else 0, "nScale": [0, 0], "nOut": [0, 0], "nConf": [0, 0]}
            ctl["nScale"][st["ts"]], ctl["nOut"][st["to"]], ctl["nConf"][st["tc"]] = (part() if st["scale"] < 1024 else 0), (part() if rng.integers(0, 4) == 0 else 0), part()
            kind, n_todo, _, _, st = hs.next_pass(st, ctl, **kw)
            if kind == "done":
                break
            assert 0 < n_todo <= nq
    assert min(planned.values()) > 20, planned


def test_next_pass_transitions():
    kw = dict(longest_mate=150)
    _, first = hs.pass_policy(**kw)
    first["nRegions"], first["regionsTotal"] = 1000, 1000 * 80000
    # a full result arena wins over everything; the other lists wait, and so do the saved regions
    kind, n, lst, clear, st = hs.next_pass(first, {"nHeavy": 5, "nHeavyLate": 2, "nScale": (3, 0), "nOut": (4, 0), "nConf": (6, 0)}, **kw)
    assert (kind, n, lst, clear) == ("out_rerun", 4, 0, 1) and (st["to"], st["heavy"], st["hoMode"], st["scale"], st["regionsTotal"]) == (1, 0, 0, 1, first["regionsTotal"])
    # ... then the gapped pass, over both heavy lists, at the gapped scale, from the saved regions, dealt out in order
    kind, n, _, _, st = hs.next_pass(st, {"nHeavy": 5, "nHeavyLate": 2, "nScale": (3, 0), "nOut": (0, 0), "nConf": (6, 0)}, **kw)
    assert (kind, n) == ("gapped", 7) and (st["heavy"], st["hoMode"], st["scale"], st["overflowScale"], st["orderedList"]) == (1, 2, 4, 4, 1)
    # ... which consumes the regions; the scale rerun goes before the confidence rerun, at four times the gapped scale
    kind, n, lst, clear, st = hs.next_pass(st, {"nScale": (3, 0), "nConf": (6, 0)}, **kw)
    assert (kind, n, lst, clear) == ("scale_rerun", 3, 0, 1)
    assert (st["ts"], st["scale"], st["overflowScale"], st["hoMode"], st["orderedList"], st["regionsTotal"], st["heavy"]) == (1, 16, 16, 0, 0, 0, 1)
    # ... the confidence rerun only when no scale rerun is pending (its list accumulates), at the scale reached
    kind, n, lst, clear, st = hs.next_pass(st, {"nScale": (0, 0), "nConf": (6, 0)}, **kw)
    assert (kind, n, lst, clear) == ("conf_rerun", 6, 0, 1) and (st["tc"], st["scale"], st["confRounds"], st["heavy"]) == (1, 16, 1, 1)
    kind, n, _, _, st = hs.next_pass(st, {}, **kw)
    assert (kind, n) == ("done", 0)
    # no gapped pass: a light pass whose reads only overflowed goes to four times the seed scale, and what it saved is dropped
    kind, n, _, _, st = hs.next_pass(first, {"nScale": (9, 0)}, **kw)
    assert (kind, n) == ("scale_rerun", 9) and (st["scale"], st["overflowScale"], st["heavy"], st["regionsTotal"]) == (4, 4, 1, 0)
    # a confidence rerun straight after the light pass runs at the gapped scale
    kind, n, _, _, st = hs.next_pass(first, {"nConf": (2, 0)}, **kw)
    assert (kind, n) == ("conf_rerun", 2) and (st["scale"], st["overflowScale"], st["heavy"], st["hoMode"], st["regionsTotal"]) == (4, 4, 1, 0, 0)
    # after a gapped pass the overflow scale is never below the gapped scale, whatever XM_GAPPED_SCALE says
    for mate in (150, 1000, 5000):
        pol, st0 = hs.pass_policy(mate)
        _, _, _, _, st = hs.next_pass(st0, {"nHeavy": 1}, longest_mate=mate)
        assert st["scale"] == pol["gappedScale"] <= st["overflowScale"]
        kind, _, _, _, st = hs.next_pass(st, {"nScale": (1, 0)}, longest_mate=mate)
        assert kind == "scale_rerun" and st["scale"] == 4 * pol["gappedScale"]


def test_next_pass_limits():
    kw = dict(longest_mate=150)
    _, st = hs.pass_policy(**kw)
    st["heavy"], st["hoMode"] = 1, 0
    st["scale"] = st["overflowScale"] = 1024
    assert hs.next_pass(st, {"nScale": (1, 0)}, **kw)[4]["scale"] == 4096
    st["scale"] = st["overflowScale"] = 4096
    with pytest.raises(RuntimeError, match=r"scratch scale limit reached \(query needs more than 4096x the default scratch\)"):
        hs.next_pass(st, {"nScale": (1, 0)}, **kw)
    st["confRounds"] = 1023
    assert hs.next_pass(st, {"nConf": (1, 0)}, **kw)[4]["confRounds"] == 1024
    st["confRounds"] = 1024
    with pytest.raises(RuntimeError, match="internal error: the confidence table does not converge"):
        hs.next_pass(st, {"nConf": (1, 0)}, **kw)


def test_no_room_behind_the_saved_reads():
    light, _, st = light_then_gapped(1000, 10, 150)
    with pytest.raises(RuntimeError, match=r"the scratch behind the saved reads is smaller than one lane's arena \(XM_SCRATCH_GIB / XM_ARENA_KB too small for this batch\)"):
        hs.plan_launch(st, 10, 1000, CUS, AMPLE, light["regionsTotal"] + 1024, longest_mate=150)


@pytest.mark.parametrize("knob,value,message", [
    ("XM_FULL_LPW", "65", "XM_FULL_LPW=65 is not valid: expected a value in 1..64"),
    ("XM_LIGHT_WAVES", "0", "XM_LIGHT_WAVES=0 is not valid: expected a value in 1..16"),
    ("XM_GAPPED_SCALE", "3", "XM_GAPPED_SCALE=3 is not valid: expected a power of two in 1..64"),
    ("XM_GAPPED_SCALE", "128", "XM_GAPPED_SCALE=128 is not valid: expected a power of two in 1..64"),
])
def test_invalid_knobs_raise(monkeypatch, knob, value, message):
    monkeypatch.setenv(knob, value)
    with pytest.raises(RuntimeError) as e:
        hs.pass_policy(150)
    assert str(e.value) == message
    if knob == "XM_GAPPED_SCALE":   # (read for batches that seed at scale 1 only; long reads have XM_GAPPED_FACTOR)
        assert hs.pass_policy(1000)[0]["gappedScale"] == 16
        monkeypatch.setenv("XM_GAPPED_FACTOR", value)
        with pytest.raises(RuntimeError, match="XM_GAPPED_FACTOR=%s is not valid" % value):
            hs.pass_policy(1000)


ARENA_NQ = (0, 1, 255, 256, 4096, 4097, 1_000_000)
ARENA_HITS = (0, 1, 2 ** 33)


def test_result_arena_sizes_equal_their_independent_statement():
    """firstArenaSize / grownArenaSize, which size every result arena of the product (ResultStage), against the formulas tests/test_gpu_result_stage.py
    sizes its overflow cases by: the first size is that of nq queries plus the replayed hits; the grown size with the cursor below, at and far above
    four times the capacity + 65536."""
    from test_gpu_result_stage import initial_int_cap, initial_dbl_cap, grown_cap
    for nq in ARENA_NQ:
        for hits in ARENA_HITS:
            assert hs.first_arena_size(nq, hits) == initial_int_cap(nq) + hits
            assert hs.first_arena_size(nq, hits, doubles=True) == initial_dbl_cap(nq) + hits
        for cap in (initial_int_cap(nq), initial_dbl_cap(nq), initial_int_cap(nq) + 2 ** 33):
            edge = 4 * cap + 65536
            for cursor in (0, cap, cap + 1, edge // 2 - 1, edge // 2, edge // 2 + 1, edge, 2 ** 40):
                assert hs.grown_arena_size(cap, cursor) == grown_cap(cap, cursor), (cap, cursor)
            assert hs.grown_arena_size(cap, edge // 2) == edge and hs.grown_arena_size(cap, edge // 2 + 1) == edge + 2 and hs.grown_arena_size(cap, 2 ** 40) == 2 ** 41


def test_first_arena_size_is_monotone():
    """more queries or more hits never start with a smaller arena, and the doubles' arena is never the larger one"""
    for doubles in (False, True):
        sizes = [[hs.first_arena_size(nq, hits, doubles) for hits in ARENA_HITS] for nq in ARENA_NQ]
        for row, above in zip(sizes, sizes[1:]):
            assert all(a < b for a, b in zip(row, above))
        for row in sizes:
            assert all(a < b for a, b in zip(row, row[1:]))
    assert all(hs.first_arena_size(nq, h, True) <= hs.first_arena_size(nq, h) for nq in ARENA_NQ for h in ARENA_HITS)
