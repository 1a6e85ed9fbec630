"""The plan and the table logic of the run-wide memory of aligned queries (mapper_amd/csrc/xm_memo_plan.h) without a GPU.  The header is plain C++ whose
functions the kernels of xm_memo.h call on the device; here tests/memo_plan_main.cpp, a stand-alone program built by this test with g++ (with
-fsanitize=address,undefined where the host compiler has the runtime), runs the same functions and is compared with restatements written here: the plan with
arithmetic, the table with a Python dict."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_BYTES = 64 << 10
DEAD = "dead"


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "memo_plan_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/memo_plan_main.cpp")
    out = str(tmp_path_factory.mktemp("memo_plan") / "memo_plan_main")
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
    """The plan restated: the largest power of two of 16-byte slots within a quarter of the budget (2^32 slots at the most), the rest (a multiple of 8) for the records."""
    if budget < MIN_BYTES:
        return 0, 0, 0
    slots = min(1 << ((budget // 4 // 16).bit_length() - 1), 1 << 32)
    return slots, (budget - 16 * slots) // 8 * 8, slots // 2


def test_plan_over_budgets(program):
    rng = np.random.default_rng(0x3E30)
    budgets = [0, 1, MIN_BYTES - 1, MIN_BYTES, MIN_BYTES + 1, 100_000, 1 << 20, (1 << 20) + 7, 64 << 20, (1 << 30) - 1, 1 << 30, 3 << 30, 40 << 30, 1 << 40]
    budgets += [int(x) for x in rng.integers(MIN_BYTES, 1 << 36, size=300)] + [int(x) for x in rng.integers(0, MIN_BYTES, size=20)]
    out = run(program, ["plan %d" % b for b in budgets])
    for b, line in zip(budgets, out):
        slots, arena, capacity, table = (int(x) for x in line.split())
        if b < MIN_BYTES:
            assert (slots, arena, capacity) == (0, 0, 0), b  # the minimum is refused
            continue
        assert slots >= 1024 and slots & (slots - 1) == 0, b
        assert table == 16 * slots and table + arena <= b and arena % 8 == 0 and b - (table + arena) < 8, b
        assert table <= b // 4 and (b // 4 < 2 * table or slots == 1 << 32), b  # the largest power of two within a quarter
        assert capacity == slots // 2, b
        assert (slots, arena, capacity) == plan_of(b), b


def test_record_layout_and_fingerprint_bits(program):
    shapes = [(150, 0, 20, 6), (150, 150, 47, 16), (1, 0, 2, 0), (7, 9, 1, 1), (1000, 0, 3, 0), (8, 8, 2, 2)]
    out = run(program, ["record %d %d %d %d" % s for s in shapes])
    for s, line in zip(shapes, out):
        at_bytes, at_ints, at_dbls, total = (int(x) for x in line.split())
        assert at_bytes == 40 and at_ints == 40 + pad8(s[0] + s[1]) and at_dbls == at_ints + pad8(4 * s[2]) and total == record_bytes(*s), s
        assert at_ints % 8 == 0 and at_dbls % 8 == 0 and total % 8 == 0
    cases = [(0xFFFFFFFFFFFFFFFF, 64), (0xFFFFFFFFFFFFFFFF, 6), (0x40, 6), (0, 64), (0x1234567890ABCDEF, 16), (0x10000, 16), (5, 1), (4, 1)]
    out = run(program, ["fp %x %d" % c for c in cases])
    for (h, bits), line in zip(cases, out):
        want = h & ((1 << bits) - 1)
        assert int(line, 16) == (want if want else 1), (h, bits)  # (never 0: that is an empty slot)


def test_parameter_change_rule(program):
    a = bytes(range(80))
    b = bytearray(a); b[79] ^= 1
    c = bytearray(a); c[0] ^= 0x80
    out = run(program, ["differ 1 %s %s" % (a.hex(), a.hex()), "differ 1 %s %s" % (a.hex(), bytes(b).hex()), "differ 1 %s %s" % (a.hex(), bytes(c).hex()),
                        "differ 0 %s %s" % (a.hex(), bytes(b).hex())])
    assert out == ["0", "1", "1", "0"]  # any bit empties a memory something was put into; an empty one takes the new parameters


class Model:
    """The memory as a dict: fingerprint -> the item stored under it, or DEAD."""

    def __init__(self, budget, bits):
        self.slots, self.arena, self.capacity = plan_of(budget)
        self.bits = bits
        self.table = {}
        self.claimed = self.cursor = self.records = 0

    def fp(self, h):
        h &= (1 << self.bits) - 1
        return h if h else 1

    def full(self):
        return self.claimed >= self.capacity or self.cursor >= self.arena

    def insert(self, items):
        n = 0 if self.full() else min(len(items), self.capacity - self.claimed)
        out = []
        for i, it in enumerate(items):
            h = self.fp(it[0])
            if i >= n:
                out.append("skipped")
            elif h in self.table:
                out.append("dropped")  # its own key is there: the first stays
            else:
                self.claimed += 1
                size = record_bytes(*it[2:])
                at, self.cursor = self.cursor, self.cursor + size
                if at + size <= self.arena:
                    self.table[h] = (it, at)
                    self.records += 1
                    out.append("stored %d" % at)
                else:
                    self.table[h] = DEAD
                    out.append("dead")
        out.append("state %d %d %d %d %d" % (self.claimed, self.cursor, self.records, min(self.cursor, self.arena), 1 if self.full() else 0))
        return out

    def lookup(self, it):
        e = self.table.get(self.fp(it[0]))
        if e is None or e == DEAD:
            return "-1"
        stored, at = e
        if stored[1] != it[1] or stored[2:4] != it[2:4]:
            return "-1"  # another query with this fingerprint
        return "%d %d %d" % (at, stored[4], stored[5])


def item_line(it):
    return "%x %d %d %d %d %d" % it


@pytest.mark.parametrize("seed,budget,bits,tiny,fills", [(1, MIN_BYTES, 64, False, True), (2, MIN_BYTES, 64, True, True), (3, 200_000, 64, False, True),
                                                         (4, 1 << 20, 6, False, False), (5, MIN_BYTES, 10, True, True), (6, 100_000, 64, True, True)])
def test_table_against_dict_model(program, seed, budget, bits, tiny, fills):
    """Seeded launches of inserts with lookups between them.  A fifth of the items take their fingerprint from a pool of 40 (different queries, equal fingerprints);
    `tiny` records (56 bytes) fill the table to its half before the arena (the half-full stop), the others fill the arena first (dead slots)."""
    rng = np.random.default_rng(0x3E00 + seed)
    model = Model(budget, bits)
    pool = [int(x) for x in rng.integers(1, 1 << 63, size=40)]
    seen, commands, want = [], ["new %d %d" % (budget, bits)], ["ok"]
    content = 0
    for launch in range(14):
        items = []
        for _ in range(int(rng.integers(1, 260))):
            content += 1
            h = pool[int(rng.integers(len(pool)))] if rng.random() < 0.2 else int(rng.integers(1, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
            if tiny:
                it = (h, content, 1, 0, 1, 0)
            else:
                paired = rng.random() < 0.4
                it = (h, content, int(rng.integers(30, 400)), int(rng.integers(30, 400)) if paired else 0, int(rng.integers(2, 120)), int(rng.integers(0, 40)))
            items.append(it)
        if launch % 5 == 4 and seen:  # something the memory may hold already, under its own fingerprint: dropped if it is there
            items.append(seen[int(rng.integers(len(seen)))])
        commands.append("insert %d" % len(items))
        commands += [item_line(it) for it in items]
        want += model.insert(items)
        seen += items
        probes = [seen[int(k)] for k in rng.integers(len(seen), size=60)]
        probes += [(it[0], it[1] + 1_000_000) + it[2:] for it in probes[:15]]                 # same fingerprint, other bytes
        probes += [(it[0], it[1], it[2] + 1) + it[3:] for it in probes[:10]]                  # same fingerprint and bytes, one base longer
        probes += [(int(rng.integers(1, 1 << 63)), 5_000_000 + k, 50, 0, 3, 0) for k in range(10)]  # never seen
        for it in probes:
            commands.append("lookup %x %d %d %d" % it[:4])
            want.append(model.lookup(it))
    got = run(program, commands)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "answer %d: program %r, model %r" % (k, g, w)
    outcomes = {w.split()[0] for w in want}
    assert {"stored", "dropped"} <= outcomes and model.claimed <= model.capacity  # (the paths this case is there for were taken)
    if fills:
        assert "skipped" in outcomes and model.full() and ("dead" in outcomes) == (not tiny)
        if tiny:
            assert model.claimed == model.capacity and model.cursor < model.arena  # stopped by the half-full rule, with room in the arena
    else:
        assert len(model.table) <= (1 << bits) and not model.full()  # 6 bits: 63 fingerprints for everything
