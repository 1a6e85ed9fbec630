"""The generations of the GPU's memory of aligned queries (xm_memory_new; mapper_amd/csrc/xm_memo_plan.h, "the memory of a GPU") without a GPU.
tests/memo_generations_main.cpp, a stand-alone program built by this test with g++ (with -fsanitize=address,undefined where the host compiler has the
runtime; nothing is loaded into python), runs align calls through the functions the kernels and xm_capi.hip call - lookup order, promotion, measure, turn,
insert - and is compared with a model written here: two dicts with byte and slot accounting.  Then the command line's flag over a stand-in database."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from mapper_amd import api, cli, synth
from standin_db import StandInDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_BYTES = 64 << 10
DEAD = "dead"


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "memo_generations_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/memo_generations_main.cpp")
    out = str(tmp_path_factory.mktemp("memo_generations") / "memo_generations_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, commands):
    r = subprocess.run([program], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def pad8(n):
    return (n + 7) & ~7


def record_bytes(len0, len1, int_len, dbl_len):
    return 40 + pad8(len0 + len1) + pad8(4 * int_len) + 8 * dbl_len


def plan_of(budget):
    """One generation's plan restated (tests/test_memo_plan.py checks it against the program of the one-generation memory)."""
    if budget < MIN_BYTES:
        return 0, 0, 0
    slots = min(1 << ((budget // 4 // 16).bit_length() - 1), 1 << 32)
    return slots, (budget - 16 * slots) // 8 * 8, slots // 2


def test_plan_over_generations_and_smallest_budgets(program):
    rng = np.random.default_rng(0x3F00)
    budgets = [0, MIN_BYTES - 1, MIN_BYTES, MIN_BYTES + 1, 2 * MIN_BYTES - 1, 2 * MIN_BYTES, 2 * MIN_BYTES + 1, 1 << 20, (1 << 20) + 9, 64 << 20, 3 << 30] + [int(x) for x in rng.integers(0, 1 << 34, size=100)]
    cases = [(b, g) for b in budgets for g in (1, 2)] + [(1 << 20, 0), (1 << 20, 3), (1 << 20, -1)]
    out = run(program, ["plan %d %d" % c for c in cases])
    for (b, g), line in zip(cases, out):
        slots, arena, capacity, smallest = (int(x) for x in line.split())
        if g not in (1, 2):
            assert (slots, arena, capacity) == (0, 0, 0), (b, g)  # one or two generations, nothing else
            continue
        assert smallest == g * MIN_BYTES
        assert (slots, arena, capacity) == plan_of(b // g), (b, g)  # every generation is the plan of its share
        assert (slots == 0) == (b < g * MIN_BYTES), (b, g)        # the smallest budget is generations * 64 KiB; less is refused
        assert g * (16 * slots + arena) <= b
    assert run(program, ["new %d 2 64" % (2 * MIN_BYTES - 1), "new %d 2 64" % (2 * MIN_BYTES), "new %d 1 64" % (MIN_BYTES - 1), "new %d 1 64" % MIN_BYTES, "new 1000000 3 64"]) == \
        ["refused", "ok", "refused", "ok", "refused"]


def test_takes_all_at_its_edges(program):
    """memoTakesAll: the young generation takes a call's n records of B bytes when claimed + n <= capacity and cursor + B <= arenaBytes - to the byte."""
    slots, arena, capacity = plan_of(MIN_BYTES)
    cases = [(0, 0, 0, 0, 1), (0, 0, capacity, arena, 1), (0, 0, capacity + 1, 8, 0), (0, 0, 1, arena + 1, 0), (capacity - 1, 0, 1, 8, 1), (capacity - 1, 0, 2, 16, 0),
             (3, arena - 400, 1, 400, 1), (3, arena - 400, 1, 401, 0), (3, arena - 399, 1, 400, 0), (capacity, arena, 0, 0, 1), (0, arena + 8, 0, 0, 0), (0, 8, 1, (1 << 64) - 8, 0)]
    out = run(program, ["takes %d %d %d %d %d" % ((MIN_BYTES,) + c[:4]) for c in cases])
    assert [int(x) for x in out] == [c[4] for c in cases]


class Generation:
    def __init__(self):
        self.table = {}  # fingerprint -> (item, offset in this generation's arena) or DEAD
        self.claimed = self.cursor = self.records = 0


class Model:
    """The memory as two dicts, with the slot and byte accounting of each generation, and the rules in the words of the issue."""

    def __init__(self, budget, generations, bits):
        self.slots, self.arena, self.capacity = plan_of(budget // generations)
        self.generations, self.bits = generations, bits
        self.gen = [Generation() for _ in range(generations)]
        self.young = 0
        self.turns = self.promoted = 0

    def fp(self, h):
        h &= (1 << self.bits) - 1
        return h if h else 1

    def takes_all(self, n, nbytes):
        y = self.gen[self.young]
        return y.claimed + n <= self.capacity and y.cursor + nbytes <= self.arena

    def find(self, it):
        """young first, then old; a key match with other bytes does not end the lookup"""
        order = [self.young] + ([1 - self.young] if self.generations == 2 else [])
        for g in order:
            e = self.gen[g].table.get(self.fp(it[0]))
            if e is not None and e != DEAD and e[0][1:4] == it[1:4]:
                return g, e[1]
        return None

    def store(self, it):
        """claim, reserve, copy - into the young generation"""
        y, h = self.gen[self.young], self.fp(it[0])
        if h in y.table:
            return "dropped"
        y.claimed += 1
        size = record_bytes(*it[2:])
        at, y.cursor = y.cursor, y.cursor + size
        if at + size > self.arena:
            y.table[h] = DEAD
            return "dead"
        y.table[h] = (it, at)
        y.records += 1
        return "stored %d" % (self.young * self.arena + at)

    def call(self, items):
        out, hits, misses = [], [], []
        for it in items:
            f = self.find(it)
            if f is None:
                out.append("-")
                misses.append(it)
            else:
                out.append("%s %d" % ("Y" if f[0] == self.young else "O", f[0] * self.arena + f[1]))
                if f[0] != self.young:
                    hits.append(it)
        # second chance: all of the old generation's hits, or none; never a turn
        if self.generations == 2 and hits and self.takes_all(len(hits), sum(record_bytes(*it[2:]) for it in hits)):
            copied = sum(1 for it in hits if self.store(it).startswith("stored"))
            self.promoted += copied
            out.append("promote %d" % copied)
        else:
            out.append("promote none")
        # insert: turn first when the young generation holds something and does not take all the call brings
        y = self.gen[self.young]
        if misses and self.generations == 2 and y.claimed > 0 and not self.takes_all(len(misses), sum(record_bytes(*it[2:]) for it in misses)):
            self.young = 1 - self.young
            self.gen[self.young] = Generation()
            self.turns += 1
            out.append("turn")
        else:
            out.append("stay")
        y = self.gen[self.young]
        full = y.claimed >= self.capacity or y.cursor >= self.arena
        take = 0 if full else min(len(misses), self.capacity - y.claimed)
        out += [self.store(it) if k < take else "skipped" for k, it in enumerate(misses)]
        g = self.gen + ([Generation()] if self.generations == 1 else [])
        held = sum(x.records for x in self.gen)
        in_use = sum(16 * self.slots + min(x.cursor, self.arena) for x in self.gen)
        out.append("state %d %d %d %d %d %d %d %d %d %d %d" % (self.young, g[0].claimed, g[0].cursor, g[0].records, g[1].claimed, g[1].cursor, g[1].records, self.turns, self.promoted, held, in_use))
        return out


def call_lines(items):
    return ["call %d" % len(items)] + ["%x %d %d %d %d %d" % it for it in items]


def check(program, model, budget, calls):
    commands, want = ["new %d %d %d" % (budget, model.generations, model.bits)], ["ok"]
    for items in calls:
        commands += call_lines(items)
        want += model.call(items)
    got = run(program, commands)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "answer %d: program %r, model %r" % (k, g, w)
    return want


def distinct_items(rng, n, first_content, tiny=False, pool=None):
    out = []
    for k in range(n):
        h = pool[int(rng.integers(len(pool)))] if pool and rng.random() < 0.25 else int(rng.integers(1, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        if tiny:
            out.append((h, first_content + k, 1, 0, 1, 0))
        else:
            paired = rng.random() < 0.4
            out.append((h, first_content + k, int(rng.integers(30, 400)), int(rng.integers(30, 400)) if paired else 0, int(rng.integers(2, 120)), int(rng.integers(0, 40))))
    return out


@pytest.mark.parametrize("seed,budget,generations,bits,tiny", [(1, 2 * MIN_BYTES, 2, 64, False), (2, 2 * MIN_BYTES, 2, 64, True), (3, 300_000, 2, 64, False), (4, 2 * MIN_BYTES, 2, 6, False),
                                                              (5, 2 * MIN_BYTES, 1, 64, False), (6, 2 * MIN_BYTES, 2, 10, True), (7, 200_000, 1, 6, False)])
def test_calls_against_the_model(program, seed, budget, generations, bits, tiny):
    """Seeded sequences of calls: new queries, queries of earlier calls (some of them aged into the old generation: served from there and promoted), empty calls,
    calls larger than a whole generation.  `tiny` records (56 bytes) fill a generation's table to its half before its arena."""
    rng = np.random.default_rng(0x3F10 + seed)
    model = Model(budget, generations, bits)
    pool = [int(x) for x in rng.integers(1, 1 << 63, size=40)]
    calls, seen, content = [], [], 1
    for k in range(40):
        kind = rng.random()
        if k % 13 == 5:
            items = []  # an empty call: nothing found, nothing promoted, no turn, nothing inserted
        elif k % 17 == 9:
            n = model.capacity + 40 if tiny else 400  # larger than a whole generation (400 records of > 128 bytes in 48 KiB .. 70 KiB): as far as room goes
            items = distinct_items(rng, n, content, tiny, pool)
        else:
            items = distinct_items(rng, int(rng.integers(1, 120 if not tiny else 300)), content, tiny, pool)
            if seen and kind < 0.6:  # with queries seen before, from every age
                back = {seen[int(i)][1]: seen[int(i)] for i in rng.integers(len(seen), size=int(rng.integers(1, 60)))}
                items += list(back.values())
        content += len(items) + 1
        items = [items[int(i)] for i in rng.permutation(len(items))]
        calls.append(items)
        seen += items
    want = check(program, model, budget, calls)
    kinds = {w.split()[0] for w in want}
    assert {"stored", "Y", "-", "stay"} <= kinds
    if generations == 2:
        assert {"turn", "O", "promote"} <= kinds and model.turns >= 2 and model.promoted > 0
        assert any(w.startswith("promote ") and w != "promote none" for w in want)
    else:
        assert "turn" not in kinds and "O" not in kinds and model.turns == 0  # one generation: nothing ever turns
        assert ("skipped" in kinds) == (bits == 64)  # full means it stops (63 fingerprints for everything never fill it)
    if bits < 64:
        assert "dropped" in kinds


def sized_items(first_content, n, size):
    """n different single reads whose records are `size` bytes each (size = 40 + pad8(len0) + pad8(4 * ints) + 8 * dbls with ints = 2, dbls = 0)"""
    len0 = size - 40 - 8
    assert len0 > 0 and len0 % 8 == 0 and record_bytes(len0, 0, 2, 0) == size
    return [(0x1000_0000_0000 + first_content + k, first_content + k, len0, 0, 2, 0) for k in range(n)]


def test_exact_fit_one_over_and_no_turn_of_an_empty_generation(program):
    budget = 2 * MIN_BYTES
    slots, arena, capacity = plan_of(MIN_BYTES)
    assert arena == 49_152 and capacity == 512
    # 96 records of 512 bytes are exactly one generation's arena: the second call of 96 does not fit beside the first, the generations turn
    a, b, c = sized_items(1, 96, 512), sized_items(1_000, 96, 512), sized_items(2_000, 95, 512)
    m = Model(budget, 2, 64)
    want = check(program, m, budget, [a, b, a, c + sized_items(3_000, 1, 512), []])
    assert [w for w in want if w in ("turn", "stay")] == ["stay", "turn", "stay", "turn", "stay"]
    assert m.turns == 2 and m.promoted == 0  # `a` was served from the old generation, and the full young one took none of it
    assert "promote none" in want and "skipped" not in want and "dead" not in want
    # one over: 95 records of 512 bytes and one of 520 are 8 bytes (the records' granule) more than a generation - into an empty young generation: no turn,
    # inserted as far as room goes (the last one finds no room); then one record of 8 bytes less beside 95: it fits exactly, no turn
    m = Model(budget, 2, 64)
    over = sized_items(1, 95, 512) + sized_items(500, 1, 520)
    want = check(program, m, budget, [over, sized_items(600, 1, 512)])
    assert [w for w in want if w in ("turn", "stay")] == ["stay", "turn"] and want.count("dead") == 1 and m.turns == 1
    m = Model(budget, 2, 64)
    want = check(program, m, budget, [sized_items(1, 95, 512), sized_items(500, 1, 512), sized_items(600, 1, 48 + 8)])
    assert [w for w in want if w in ("turn", "stay")] == ["stay", "stay", "turn"] and m.gen[1 - m.young].cursor == arena
    # larger than a whole generation, twice: the first into the empty young generation (no turn of an empty generation), the second turns once and is cut as well
    m = Model(budget, 2, 64)
    want = check(program, m, budget, [sized_items(1, 150, 512), sized_items(1_000, 150, 512), sized_items(1, 150, 512)])
    assert [w for w in want if w in ("turn", "stay")] == ["stay", "turn", "turn"] and m.turns == 2
    assert want.count("dead") >= 2 and all(x.records <= 96 for x in m.gen)
    # one generation of the same total budget: never a turn, and what does not fit is not remembered
    m = Model(budget, 1, 64)
    want = check(program, m, budget, [sized_items(1, 150, 512), sized_items(1_000, 150, 512), sized_items(1, 150, 512)])
    assert "turn" not in want and m.turns == 0 and m.gen[0].records == plan_of(budget)[1] // 512


def test_lookup_order_with_one_fingerprint_for_two_queries(program):
    """Six bits of fingerprint.  Query A ages into the old generation; query B, with A's fingerprint, is then remembered in the young one.  A's lookup meets B's
    key and record in the young table, which is not A - and still finds A in the old generation.  Its promotion meets its own key in the young table and is
    dropped.  A query held in both generations is served from the young one."""
    budget = 2 * MIN_BYTES
    a = (0x40 + 5, 1, 152, 0, 2, 0)
    b = (0x80 + 5, 2, 152, 0, 2, 0)   # a's six bits, other bytes
    c = (0x40 + 9, 3, 152, 0, 2, 0)
    big1 = (0x40 + 17, 4, 40_000, 0, 2, 0)  # 40 048 bytes of a generation's 49 152: two of them do not fit one generation
    big2 = (0x40 + 18, 5, 40_000, 0, 2, 0)
    m = Model(budget, 2, 6)
    calls = [[a, c], [big1], [big2], [b], [a], [c], [c], [a, b]]
    want = check(program, m, budget, calls)
    assert [w for w in want if w in ("turn", "stay")] == ["stay", "stay", "turn", "stay", "stay", "stay", "stay", "stay"] and m.turns == 1
    answers = [w.split()[0] for w in want if w[0] in "YO-"]
    #                  a    c    big1 big2 b    a    c    c    a    b
    assert answers == ["-", "-", "-", "-", "-", "O", "O", "Y", "O", "Y"]
    # b was a miss in both generations (the old one holds its key with a's bytes) and went into the young one; a is then served from the OLD generation although
    # the young table holds its key, and its promotion is dropped; c's is not; c is then held in both and served from the young one
    assert [w for w in want if w.startswith("promote")] == ["promote none"] * 4 + ["promote 0", "promote 1", "promote none", "promote 0"] and m.promoted == 1
    assert want.count("dropped") == 0 and want.count("dead") == 0


def test_parameter_change_empties_every_generation(program):
    budget = 2 * MIN_BYTES
    a, b = sized_items(1, 96, 512), sized_items(1_000, 50, 512)
    got = run(program, ["new %d 2 64" % budget] + call_lines(a) + call_lines(b) + ["empty"] + call_lines(a + b))
    lookups = [g for g in got if g[0] in "YO-"]
    assert lookups[-len(a + b):] == ["-"] * len(a + b)  # neither generation holds anything
    assert "Y" not in {g[0] for g in lookups} and got.count("turn") == 1  # (b did not fit beside a: a was in the old generation, b in the young one)
    young, c0, u0, r0, c1, u1, r1 = (int(x) for x in got[-1].split()[1:8])
    # into the emptied young generation as far as room goes: all 146 claim a slot and move the cursor, 96 find room for their record (the others' slots stay dead)
    assert sorted([(c0, u0, r0), (c1, u1, r1)]) == [(0, 0, 0), (146, 146 * 512, 96)]


# ---- the command line: --remember-queries-per-gpu over a stand-in database
class SharedStandIn(StandInDatabase):
    """a stand-in that takes the keyword of the per-GPU memory and records what the command line handed in"""

    def __init__(self, *args, shared_memo_bytes=0, per_context_extra=0, **kw):
        super().__init__(*args, per_context_extra=per_context_extra, **kw)
        self.shared_memo_bytes, self.per_context_extra = shared_memo_bytes, per_context_extra


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("memo_generations_cli")
    dec = np.frombuffer(b"?ACMGRSVTWYHKDBN", dtype=np.uint8)
    ref = synth.synthetic_reference(12_000, seed=0xEC011)
    (d / "ref.fa").write_text(">chrA\n%s\n" % dec[ref].tobytes().decode())
    reads = synth.synthetic_single_end(ref, 40, seed=5)[0]
    (d / "se.fq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, dec[r].tobytes().decode(), "I" * len(r)) for i, r in enumerate(reads)))
    return ["--reference", str(d / "ref.fa"), "--queries", str(d / "se.fq"), "--no-output", "--batch-size", "16"]


def test_flag_is_parsed_and_counted_once_per_gpu(job, capsys):
    o = cli.parse_args(job + ["--remember-queries-per-gpu", "8"])
    assert o["remember_per_gpu"] == 8 << 20 and not o.get("remember")
    StandInDatabase.opened.clear()
    assert cli.run(job + ["--remember-queries-per-gpu", "8", "--contexts", "3"], out=io.StringIO(), open_database=SharedStandIn) == 0
    db = StandInDatabase.opened[-1]
    assert db.closed and db.devices == [0, 0, 0]
    assert db.shared_memo_bytes == 8 << 20 and db.per_context_extra == 0  # the GPU's memory is no part of what every context allocates beside its scratch
    err = capsys.readouterr().err
    assert err.count("Remembered queries: ") == 1 and " of 40 queries " in err
    # the per-context flag is counted per context, and a job without either flag hands in neither keyword (the plain stand-in takes none)
    StandInDatabase.opened.clear()
    assert cli.run(job, out=io.StringIO(), open_database=StandInDatabase) == 0
    assert "Remembered queries" not in capsys.readouterr().err

    class PerContext(StandInDatabase):
        def __init__(self, *args, memo_bytes=0, per_context_extra=0, **kw):
            super().__init__(*args, per_context_extra=per_context_extra, **kw)
            self.memo_bytes, self.per_context_extra = memo_bytes, per_context_extra

    assert cli.run(job + ["--remember-queries", "8", "--contexts", "3"], out=io.StringIO(), open_database=PerContext) == 0
    db = StandInDatabase.opened[-1]
    assert db.memo_bytes == 8 << 20 and db.per_context_extra == 8 << 20


def test_both_flags_are_a_usage_error(job):
    for extra in (["--remember-queries", "8", "--remember-queries-per-gpu", "8"], ["--remember-queries-per-gpu", "8", "--remember-queries", "64"]):
        with pytest.raises(cli.UsageError):
            cli.parse_args(job + extra)
    with pytest.raises(cli.UsageError):
        cli.parse_args(job + ["--remember-queries-per-gpu", "-1"])
    assert cli.main(job + ["--remember-queries", "8", "--remember-queries-per-gpu", "8"]) == 1
    from mapper_amd import multi
    with pytest.raises(ValueError):
        multi.MultiGpuDatabase([("c", np.ones(10, np.uint8))], [0, 0], memo_bytes=1 << 20, shared_memo_bytes=1 << 20)


def test_divide_scratch_counts_the_shared_memory_once(monkeypatch):
    """api.divide_scratch: what a GPU allocates once comes off what is free before the contexts divide it; what every context allocates comes off per context."""
    class Context:
        def set_scratch(self, n):
            self.scratch = n

    free = 100 << 30
    monkeypatch.setattr(api, "device_memory", lambda device=0: (free, 288 << 30))
    ctx = [Context() for _ in range(3)]
    reserve = 24 << 30
    n0, plain = api.divide_scratch(ctx, 0)
    n1, shared = api.divide_scratch(ctx, 0, shared_extra=6 << 30)
    n2, each = api.divide_scratch(ctx, 0, per_context_extra=6 << 30)
    assert (n0, n1, n2) == (3, 3, 3)
    assert plain == (free - reserve) // 3 and shared == (free - reserve - (6 << 30)) // 3 and each == (free - reserve - 3 * (6 << 30)) // 3
    assert plain - shared == (6 << 30) // 3 and plain - each == 6 << 30 and all(c.scratch == each for c in ctx)
