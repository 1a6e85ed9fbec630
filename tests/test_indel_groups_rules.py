"""The grouping of the pile-up's indel events without a GPU: the rules the kernels of xm_indel_groups.h apply (mapper_amd/csrc/xm_indel_groups_rules.h, plain
C++) run by tests/indel_groups_rules_main.cpp - a sequential restatement of the fold, built here with g++ (with -fsanitize=address,undefined where the host
compiler has the runtime) - against the definition, pileup.CountedMatchDatabase._indels() over the same events; the command line's --group-indels-on-gpu: what
it accepts and refuses, and the job over a database and a pile-up that need no GPU.  Groups are compared for equality as dicts."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import indel_groups_cases as gc
import pileup_workloads as W
from mapper_amd import api, cli, pileup
from pileup_model import PileupModel
from standin_db import StandInDatabase
from test_mutations_rules import KeepingDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = gc.UNIT


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "indel_groups_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/indel_groups_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("indel_groups_rules") / "indel_groups_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def folded(program, path, calls, bits=64, capacity=4):
    """The program's fold of the calls -> ({key: units} of its groups, [(call, event, letters)] left over, (table, record, arena) growths, groups found again)."""
    with open(path, "w") as case:
        case.write("bits %d\ncapacity %d\ncalls %d\n" % (bits, capacity, len(calls)))
        for call in calls:
            case.write("events %d\n" % len(call))
            for e, text in call:
                case.write("%s %s\n" % (" ".join(str(int(x)) for x in e), text or "-"))
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    groups, left, grows, found = {}, [], None, None
    for l in (l.split() for l in r.stdout.splitlines()):
        if l[0] == "group":
            key = gc.group_key(int(l[1]), int(l[2]), int(l[3]), int(l[4]), "" if l[6] == "-" else l[6])
            assert key not in groups, key   # a key has one group
            groups[key] = int(l[5])
        elif l[0] == "left":
            left.append((int(l[1]), tuple(int(x) for x in l[2:10]), "" if l[10] == "-" else l[10]))
        elif l[0] == "grows":
            grows = tuple(int(x) for x in l[1:])
        elif l[0] == "found":
            found = int(l[1])
    return groups, left, grows, found


def union(groups, left):
    """The device's groups and the host's groups of the left-overs, which must not share a key -> the sum of both."""
    host = gc.definition([[(e, text) for _, e, text in left]])
    assert not set(host) & set(groups)
    return {**groups, **host}


def check(program, tmp_path, calls, **knobs):
    groups, left, grows, found = folded(program, str(tmp_path / "case.txt"), calls, **knobs)
    assert union(groups, left) == gc.definition(calls)
    return groups, left, grows, found


# ---------------------------------------------------------------- against the definition
def test_insertions_that_differ_only_in_their_last_letter_or_only_in_length(program, tmp_path):
    long_a, long_b = "ACGT" * 5 + "A", "ACGT" * 5 + "C"
    calls = [[gc.insertion(0, 7, "ACGTACGA"), gc.insertion(0, 7, "ACGTACGC"), gc.insertion(0, 7, "ACGTACGA", 2 * UNIT), gc.insertion(0, 7, long_a), gc.insertion(0, 7, long_b),
              gc.insertion(0, 7, "ACGTACG"), gc.insertion(0, 7, "ACGTACGAA"), gc.insertion(0, 7, "A"), gc.insertion(0, 7, "AA"), gc.insertion(2, 7, "A")]]
    groups, left, _, _ = check(program, tmp_path, calls)
    assert not left and len(groups) == 9 and groups[(0, 7, 1, "-" * 8, "ACGTACGA")] == 3 * UNIT and groups[(0, 7, 1, "-" * 8, "ACGTACGC")] == UNIT


def test_a_deletion_and_an_insertion_at_one_position(program, tmp_path):
    """An insertion at startB and a deletion at startB - 1 share pos1; the kind keeps them apart, and so does the length of two deletions."""
    calls = [[gc.insertion(0, 20, "GG"), gc.deletion(0, 19, 2), gc.deletion(0, 19, 3), gc.deletion(0, 20, 2), gc.insertion(0, 20, "GG"), gc.deletion(0, 19, 2, UNIT // 2)]]
    groups, left, _, _ = check(program, tmp_path, calls)
    assert not left and sorted((k[1], k[2], max(len(k[3]), len(k[4])), w) for k, w in groups.items()) == [(20, 1, 2, 2 * UNIT), (20, 2, 2, UNIT + UNIT // 2), (20, 2, 3, UNIT), (21, 2, 2, UNIT)]


def test_flagged_events_are_in_no_group(program, tmp_path):
    calls = [[gc.insertion(0, 5, "AC", flags=4), gc.insertion(0, 5, "AC", flags=6), gc.insertion(0, 5, "AC", flags=3), gc.deletion(0, 9, 1, flags=5), gc.deletion(2, 9, 1, flags=4)]]
    groups, left, _, _ = check(program, tmp_path, calls)
    assert not left and groups == {(0, 5, 1, "--", "AC"): UNIT}
    calls = gc.random_calls(200, seed=3, flagged=0.4)
    groups, _, _, _ = check(program, tmp_path, calls)
    assert 0 < len(groups) < len(gc.definition([[(e[:5] + (0,) + e[6:], t) for e, t in calls[0]]]))   # groups of flagged events alone are gone


def test_one_key_in_three_calls(program, tmp_path):
    calls = [[gc.insertion(2, 40, "TTT"), gc.deletion(0, 3, 4)], [gc.deletion(0, 4, 4), gc.insertion(2, 40, "TTT", UNIT // 2)], [gc.insertion(2, 40, "TTT", 3 * UNIT), gc.insertion(2, 40, "TTA")]]
    groups, left, _, _ = check(program, tmp_path, calls)
    assert not left and groups[(2, 40, 1, "---", "TTT")] == 4 * UNIT + UNIT // 2 and len(groups) == 4


@pytest.mark.parametrize("seed", [1, 2])
def test_with_two_bits_of_fingerprint_collisions_are_the_rule(program, tmp_path, seed):
    """Four fingerprints for some hundred keys: at most four groups on the device, everything else is left over - and grouped by the host to the same sums."""
    calls = gc.random_calls(300, seed=seed, num_calls=3, flagged=0.1)
    groups, left, _, _ = check(program, tmp_path, calls, bits=2)
    assert len(left) > 0 and 0 < len(groups) <= 4
    assert {c for c, _, _ in left} == {0, 1, 2}
    whole, none, _, _ = check(program, tmp_path, calls, bits=64)
    assert not none and len(whole) > 50


# ---------------------------------------------------------------- growth
def test_growth_from_four_slots_finds_every_key_again(program, tmp_path):
    calls = gc.distinct_calls(700, num_calls=7)
    groups, left, grows, found = check(program, tmp_path, calls, capacity=4)
    assert not left and len(groups) == 700
    assert grows[0] >= 3 and grows[1] >= 3 and found >= 100 + 200 + 300   # (the program looked every group up behind every growth of the table)
    calls = [[gc.insertion(0, k, gc.random_letters(np.random.default_rng(k), 1 + 37 * k)) for k in range(3 * c, 3 * c + 3)] for c in range(5)]
    groups, left, grows, _ = check(program, tmp_path, calls, capacity=4)
    assert not left and len(groups) == 15 and grows[2] >= 3   # the arena grew and kept its letters


# ---------------------------------------------------------------- the command line
def test_cli_flag_and_what_it_needs():
    ref, q, mut = ["--reference", "r.fa"], ["--queries", "q.fq"], ["--out-mutations", "m.txt"]
    o = cli.parse_args(ref + q + mut + ["--group-indels-on-gpu"])
    assert o["group_indels_on_gpu"] is True and not cli.needs_objects(o) and not o.get("call_mutations_on_gpu")
    assert not cli.parse_args(ref + q + mut).get("group_indels_on_gpu")
    assert not cli.parse_args(ref + q + mut + ["--call-mutations-on-gpu"]).get("group_indels_on_gpu")   # (independent of each other)
    for ok in (["--call-mutations-on-gpu"], ["--gpus", "2"], ["--contexts", "2"], ["--parse-on-gpu"], ["--out-sam", "o.sam"],
               ["--call-mutations-on-gpu", "--out-sam", "o.sam", "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"],
               ["--out-refs-map-count", "c.txt", "--count-refs-on-gpu"], ["--distinguish-query-ends", "0"]):
        assert cli.parse_args(ref + q + mut + ok + ["--group-indels-on-gpu"])["group_indels_on_gpu"] is True, ok
    for flags, message in ((["--out-sam", "o.sam", "--group-indels-on-gpu"], "--group-indels-on-gpu has nothing to do without --out-mutations"),
                           (["--no-output", "--group-indels-on-gpu"], "--group-indels-on-gpu has nothing to do without --out-mutations"),
                           (mut + ["--group-indels-on-gpu", "--per-object"], "--group-indels-on-gpu and --per-object exclude each other"),
                           (mut + ["--group-indels-on-gpu", "--out-refs-map-count", "c.txt"], "--group-indels-on-gpu and --out-refs-map-count exclude each other")):
        with pytest.raises(cli.UsageError, match=message):
            cli.parse_args(ref + q + flags)
    with pytest.raises(cli.UsageError, match="--format-on-gpu and --out-mutations exclude each other"):   # (the flag alone does not lift the rule)
        cli.parse_args(ref + q + mut + ["--out-sam", "o.sam", "--format-on-gpu", "--group-indels-on-gpu"])


class GroupingMatchDatabase(pileup.CountedMatchDatabase):
    """pileup.MatchDatabase for the command line without a GPU: the plain recount (tests/pileup_model.py) piles up what the stand-in aligned.  Asked to group, the
    events of every add_last are a call of the rules' program, and _indels() is its groups and the groups of what it left over."""
    program, tmp, made = None, None, []

    def __init__(self, database, query_end_fraction=0.0, keep_insert_text=False, group_on_gpu=False):
        self.db, self.model, self.mates, self.group_on_gpu, self.cuts = database, PileupModel(database.contigs, query_end_fraction), [], group_on_gpu, [0]
        self.contigs, self.query_end_fraction, self._L, self._h = database.contigs, float(query_end_fraction), None, []
        GroupingMatchDatabase.made.append(self)

    def add_last(self, queries=None, replica=0):
        assert queries is None   # (a streamed job hands no queries in)
        batch, result = self.db.last
        self.mates.append([[m.copy() for m in q] for q in W.mates_of(batch)])
        n = self.model.add([result.query_alignments(q) for q in range(batch.nq)], self.mates[-1])
        self.cuts.append(len(self.model.sorted_events()))
        return n

    def mutations(self, parameters=None, on_gpu=False):
        m = self.model
        fed = pileup.CountedMatchDatabase(m.contigs, m.depth, m.alt, m.middle, m.sorted_events(), self.mates, m.f)
        want = fed._indels()
        if self.group_on_gpu:
            events = sorted(m.sorted_events(), key=lambda e: e[4])   # (query ordinals ascend with the batches)
            items = []
            for e in events:
                text = ""
                if e[2] == 1:
                    mate = fed._mate(0, e[4], e[5] & 1)
                    text = api.decode((api.reverse_complement(mate) if (e[5] >> 1) & 1 else mate)[e[6]:e[6] + e[3]])
                items.append((tuple(int(x) for x in e), text))
            firsts = np.cumsum([0] + [len(b) for b in self.mates])
            calls = [[it for it in items if firsts[k] <= it[0][4] < firsts[k + 1]] for k in range(len(self.mates))]
            groups, left, _, _ = folded(self.program, os.path.join(self.tmp, "job.txt"), calls)
            assert not left and len(calls) >= 3 and sum(len(c) for c in calls) == len(events) > 50
            contigs = fed.contigs
            got = {}
            for (c, pos1, kind, ra, qa), w in groups.items():   # (the keys of gc.group_key are over the cases' own contigs: the deletions' alleles are this job's)
                got[(c, pos1, kind, api.decode(contigs[c][1][pos1 - 1:pos1 - 1 + len(qa)]) if kind == 2 else ra, qa)] = w
            assert got == want
            fed._indels = lambda: dict(sorted(got.items()))
        return fed.mutations(parameters)

    def close(self):
        pass


def test_the_job_with_the_flag_writes_the_host_paths_file(program, tmp_path, monkeypatch):
    from mapper_amd import synth
    ref = synth.synthetic_reference(6_000, seed=0xEC011)
    (tmp_path / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n" % (api.decode(ref[:4_000]), api.decode(ref[4_000:])))
    reads = list(synth.synthetic_single_end(ref[:4_000], 160, seed=5, indel_prob=0.5)[0]) + list(synth.synthetic_single_end(ref[4_000:], 80, seed=6, indel_prob=0.5)[0])
    (tmp_path / "se.fq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)) for i, r in enumerate(reads)))
    monkeypatch.setattr(pileup, "MatchDatabase", GroupingMatchDatabase)
    GroupingMatchDatabase.program, GroupingMatchDatabase.tmp = program, str(tmp_path)
    job = ["--reference", str(tmp_path / "ref.fa"), "--queries", str(tmp_path / "se.fq"), "--batch-size", "64", "--contexts", "1"]
    for thresholds in ([], ["--snp-threshold", "0", "0", "--indel-threshold", "0", "0"]):
        outs = {}
        for mode, flags in (("host", []), ("grouped", ["--group-indels-on-gpu"])):
            StandInDatabase.opened.clear()
            del GroupingMatchDatabase.made[:]
            path, log = str(tmp_path / (mode + ".txt")), io.StringIO()
            assert cli.run(job + ["--out-mutations", path] + thresholds + flags, out=log, open_database=KeepingDatabase) == 0
            assert [m.group_on_gpu for m in GroupingMatchDatabase.made] == [mode == "grouped"] and StandInDatabase.opened[0].closed
            outs[mode] = (open(path, "rb").read(), log.getvalue())
        assert outs["grouped"] == outs["host"]
        body = [l.split(b"\t") for l in outs["host"][0].split(b"\n") if l and not l.startswith(b"#") and not l.startswith(b"CHR")]
        if thresholds:   # everything: insertions and deletions on both contigs
            assert len(body) > 100 and any(set(l[2]) == {ord("-")} for l in body) and any(set(l[3]) == {ord("-")} for l in body)
