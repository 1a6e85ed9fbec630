"""The thresholds of the mutations file without a GPU: the rules the kernels of xm_mutations.h apply (mapper_amd/csrc/xm_mutations_rules.h, plain C++) run by
tests/mutations_rules_main.cpp, a stand-alone program built here with g++ (with -fsanitize=address,undefined where the host compiler has the runtime), against
the host path - pileup.CountedMatchDatabase.mutations() over the same counts; the command line's --call-mutations-on-gpu: what it accepts and refuses, and the
job over a database and a pile-up that need no GPU.  Rows are compared for equality, never within a tolerance."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import mutations_cases as mc
import oracle_lib
import pileup_workloads as W
from mapper_amd import _capi, api, cli, pileup
from pileup_model import PileupModel
from standin_db import StandInDatabase

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = mc.UNIT


def _compile(out, flags):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "mutations_rules_main.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/mutations_rules_main.cpp")
    out = str(tmp_path_factory.mktemp("mutations_rules") / "mutations_rules_main")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(out, [])  # (no sanitizer runtime beside this compiler)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def judged(program, path, lengths, depth, alt, middle, f, candidates):
    """The program's answer for the case -> (xm_snp_row records, xm_indel_verdict records)."""
    with open(path, "w") as case:
        case.write("filter %r %r %r %r %r %r\n" % (f.minSNPTotalDepth, f.minIndelTotalStartDepth, f.minIndelContinuationTotalDepth, f.minSNPDepthFraction,
                                                  f.minIndelStartDepthFraction, f.minIndelContinuationDepthFraction))
        case.write("contigs %d %s\n" % (len(lengths), " ".join(str(n) for n in lengths)))
        case.write("counts %d\n" % len(depth))
        for a in (depth, alt.reshape(-1), middle):
            case.write(" ".join(str(int(x)) for x in a) + "\n")
        case.write("candidates %d\n" % len(candidates))
        for c in candidates:
            case.write("%d %d %d %d %d\n" % (c["contig"], c["kind"], c["pos1"], c["length"], c["support_units"]))
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    snps = mc.snp_array([(int(l[1]), int(l[2]), int(l[3]), 0, int(l[4]), int(l[5])) for l in lines if l[0] == "snp"])
    verdicts = np.array([(int(l[1]), int(l[2])) for l in lines if l[0] == "verdict"], _capi.INDEL_VERDICT).reshape(-1)
    assert len(snps) + len(verdicts) == len(lines) and len(verdicts) == len(candidates)
    return snps, verdicts


def check(program, tmp_path, lengths, depth, alt, middle, f, events=(), fraction=0.0):
    """The host's rows for the counts, after the rules' program gave the same -> (rows, verdicts by (contig, pos1, kind, length))."""
    fed = mc.counted(lengths, depth, alt, middle, events, fraction)
    want = fed.mutations(f)
    indels = list(fed._indels().items())
    snps, verdicts = judged(program, str(tmp_path / "case.txt"), lengths, depth, alt, middle, f, pileup.indel_candidates(indels))
    assert mc.rows_from(fed, snps, indels, verdicts) == want
    return want, {key[:3] + (max(len(key[3]), len(key[4])),): (int(v["total_units"]), int(v["keep"])) for (key, _), v in zip(indels, verdicts)}


# ---------------------------------------------------------------- the SNP pair
def test_seven_of_ten_at_seven_tenths_is_kept_and_so_is_the_case_that_needs_the_float_product(program, tmp_path):
    """pileup.py's documented case - 0.7 of a depth of 10 is 7.0 in float - and one that tells the float32 product from the double product of the narrowed
    fraction: float32(0.6) is above 0.6, ten times it is 6.0000002 in double (6 of 10 would be dropped) and rounds to 6.0 in float32 (it is kept)."""
    depth, alt, middle = mc.empty_counts(3)
    depth[:] = 10 * UNIT
    alt[0, 0] = 7 * UNIT   # A at position 0
    alt[2, 1] = 6 * UNIT   # G at position 1
    alt[3, 2] = 6 * UNIT - 1
    assert float(np.float32(0.6)) * 10 > 6 and np.float32(0.6) * np.float32(10) == np.float32(6)
    rows, _ = check(program, tmp_path, [3], depth, alt, middle, mc.Filter(0.0, 0.7))
    assert [(r[1], r[3], r[4]) for r in rows] == [(1, "A", 7.0)]
    rows, _ = check(program, tmp_path, [3], depth, alt, middle, mc.Filter(0.0, 0.6))
    assert [(r[1], r[3]) for r in rows] == [(1, "A"), (2, "G")]   # (one unit below 6 reads is below)


def test_totals_just_below_and_at_the_snp_total_depth(program, tmp_path):
    depth, alt, middle = mc.empty_counts(4)
    depth[:] = [5 * UNIT - 1, 5 * UNIT, 5 * UNIT + 1, 0]
    alt[1, :] = [UNIT, UNIT, UNIT, UNIT]   # (an alt at a position without depth: kept by a filter without thresholds only)
    rows, _ = check(program, tmp_path, [4], depth, alt, middle, mc.Filter(5.0, 0.0))
    assert [r[1] for r in rows] == [2, 3]
    rows, _ = check(program, tmp_path, [4], depth, alt, middle, mc.Filter.emptyFilter())
    assert [r[1] for r in rows] == [1, 2, 3, 4]


def test_rows_are_ordered_by_contig_position_and_letter(program, tmp_path):
    lengths = [3, 1, 2]
    depth, alt, middle = mc.random_counts(6, 1.0, seed=3)
    rows, _ = check(program, tmp_path, lengths, depth, alt, middle, mc.Filter.emptyFilter())
    assert [(r[0], r[1], r[3]) for r in rows] == [(c, p + 1, b) for c, n in enumerate(lengths) for p in range(n) for b in "ACGT"]


# ---------------------------------------------------------------- indels
INDEL_FILTER = mc.Filter(0.0, 0.0, 2.0, 0.5, 2.0, 0.5)   # two reads of middle depth and half of it, at the start and at every further base


def deletion(contig, start, length, weight=4 * UNIT, flags=0):
    return (contig, start, 2, length, 0, flags, 10, weight)


def insertion(contig, start, length, weight=4 * UNIT, flags=0):
    return (contig, start, 1, length, 0, flags, 10, weight)


def test_a_deletion_is_cut_where_its_continuation_fails(program, tmp_path):
    depth, alt, middle = mc.empty_counts(40)
    depth[:] = 8 * UNIT
    middle[:] = 6 * UNIT
    middle[11] = UNIT            # the 2nd base of the deletion at 10: below two reads
    middle[23] = 9 * UNIT        # the last base of the deletion at 20: the support is less than half of it
    events = [deletion(0, 10, 4), deletion(0, 20, 4), deletion(0, 30, 4), deletion(0, 35, 1)]
    rows, verdicts = check(program, tmp_path, [40], depth, alt, middle, INDEL_FILTER, events)
    assert verdicts == {(0, 11, 2, 4): (6 * UNIT, 1), (0, 21, 2, 4): (6 * UNIT, 3), (0, 31, 2, 4): (6 * UNIT, 4), (0, 36, 2, 1): (6 * UNIT, 1)}
    assert [(r[1], len(r[2]), r[3]) for r in rows] == [(11, 1, "-"), (21, 3, "---"), (31, 4, "----"), (36, 1, "-")]


def test_a_candidate_below_the_start_pair_is_dropped(program, tmp_path):
    depth, alt, middle = mc.empty_counts(20)
    depth[:] = 20 * UNIT
    middle[:] = 6 * UNIT
    middle[5] = 2 * UNIT - 1     # below two reads
    middle[9] = 9 * UNIT         # four reads are less than half of nine
    events = [deletion(0, 5, 2), deletion(0, 9, 2), insertion(0, 12, 2)]
    rows, verdicts = check(program, tmp_path, [20], depth, alt, middle, INDEL_FILTER, events)
    assert verdicts == {(0, 6, 2, 2): (2 * UNIT - 1, 0), (0, 10, 2, 2): (9 * UNIT, 0), (0, 12, 1, 2): (6 * UNIT, 2)}
    assert [(r[1], r[2]) for r in rows] == [(12, "--")]


def test_a_deletion_that_runs_to_the_last_base_of_a_contig_stays_in_it(program, tmp_path):
    """Contig 0 ends at a high middle depth and contig 1 starts without any: a deletion over the last three bases of contig 0 is whole, and so is one whose
    length overruns the end (its further bases are all judged at the last base), where a walk into contig 1 would cut both."""
    lengths = [10, 6]
    depth, alt, middle = mc.empty_counts(16)
    depth[:] = 8 * UNIT
    middle[:10] = 6 * UNIT
    events = [deletion(0, 7, 3), deletion(0, 8, 4, weight=3 * UNIT), deletion(1, 0, 2)]
    rows, verdicts = check(program, tmp_path, lengths, depth, alt, middle, INDEL_FILTER, events)
    assert verdicts == {(0, 8, 2, 3): (6 * UNIT, 3), (0, 9, 2, 4): (6 * UNIT, 4), (1, 1, 2, 2): (0, 0)}
    assert [(r[0], r[1], len(r[2]), r[3]) for r in rows] == [(0, 8, 3, "---"), (0, 9, 2, "----")]   # (the reference has two bases for the second)


def test_insertions_at_position_zero_and_at_the_last_base(program, tmp_path):
    """An insertion in front of the first base has pos1 = 0 and is judged at base 0; one behind the last base is judged at the last base; every further base
    of an insertion is judged at that one position."""
    lengths = [8, 5]
    depth, alt, middle = mc.empty_counts(13)
    depth[:] = 8 * UNIT
    middle[:] = UNIT             # below two reads everywhere ...
    middle[[0, 7, 8, 12]] = 6 * UNIT   # ... but at the first and last base of both contigs
    events = [insertion(0, 0, 3), insertion(0, 8, 3), insertion(1, 0, 2), insertion(1, 5, 4), insertion(0, 4, 2), insertion(1, 4, 2)]
    rows, verdicts = check(program, tmp_path, lengths, depth, alt, middle, INDEL_FILTER, events)
    assert verdicts == {(0, 0, 1, 3): (6 * UNIT, 3), (0, 8, 1, 3): (6 * UNIT, 3), (1, 0, 1, 2): (6 * UNIT, 2), (1, 5, 1, 4): (6 * UNIT, 4), (0, 4, 1, 2): (UNIT, 0), (1, 4, 1, 2): (UNIT, 0)}
    assert [(r[0], r[1], r[2]) for r in rows] == [(0, 0, "---"), (0, 8, "---"), (1, 0, "--"), (1, 5, "----")]


@pytest.mark.parametrize("fraction", [0.0, 0.1])
def test_with_and_without_a_query_end_fraction(program, tmp_path, fraction):
    """Without a fraction the middle depth is the depth; with one it is its own array, and the events near a query end support nothing."""
    lengths = [63, 1, 64]
    depth, alt, middle = mc.random_counts(128, 0.2, seed=11)
    if fraction == 0:
        middle = depth.copy()
    events = mc.random_events(lengths, 60, seed=12, flagged=0.3 if fraction else 0.0)
    for name, f in mc.filters().items():
        rows, verdicts = check(program, tmp_path, lengths, depth, alt, middle, f, events, fraction)
        if name == "empty":
            everything = len(rows)
            assert len(verdicts) > 30 and all(keep > 0 for _, keep in verdicts.values())
            assert (len(verdicts) < len(set(e[:4] for e in events))) == (fraction > 0)   # groups of flagged events alone are gone
        if name == "half":
            kept = sum(1 for _, keep in verdicts.values() if keep > 0)
            assert 0 < kept < len(verdicts) and 0 < len(rows) < everything


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_counts_in_units_that_are_no_whole_reads(program, tmp_path, seed):
    lengths = [40, 17, 1, 30]
    depth, alt, middle = mc.random_counts(88, 0.5, seed=seed, whole_reads=False)
    events = mc.random_events(lengths, 50, seed=seed + 20)
    sizes = [len(check(program, tmp_path, lengths, depth, alt, middle, f, events, 0.1)[0]) for f in mc.filters().values()]
    assert sizes[0] > sizes[2] > sizes[1] >= 0


# ---------------------------------------------------------------- the command line
def test_cli_flag_and_what_it_needs():
    ref, q, mut = ["--reference", "r.fa"], ["--queries", "q.fq"], ["--out-mutations", "m.txt"]
    o = cli.parse_args(ref + q + mut + ["--call-mutations-on-gpu"])
    assert o["call_mutations_on_gpu"] is True and not cli.needs_objects(o)
    assert not cli.parse_args(ref + q + mut).get("call_mutations_on_gpu")
    for ok in (["--gpus", "2"], ["--contexts", "2"], ["--devices", "0,0"], ["--parse-on-gpu"], ["--parse-on-gpu", "--results-on-gpu"], ["--out-sam", "o.sam"],
               ["--out-sam", "o.sam", "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"], ["--out-unaligned", "u.fq", "--parse-on-gpu", "--results-on-gpu", "--unaligned-on-gpu", "--batch-on-gpu"],
               ["--snp-threshold", "3", "0.5", "--distinguish-query-ends", "0"]):
        assert cli.parse_args(ref + q + mut + ok + ["--call-mutations-on-gpu"])["call_mutations_on_gpu"] is True, ok
    for flags, message in ((["--out-sam", "o.sam", "--call-mutations-on-gpu"], "--call-mutations-on-gpu has nothing to do without --out-mutations"),
                           (["--no-output", "--call-mutations-on-gpu"], "--call-mutations-on-gpu has nothing to do without --out-mutations"),
                           (mut + ["--call-mutations-on-gpu", "--per-object"], "--call-mutations-on-gpu and --per-object exclude each other")):
        with pytest.raises(cli.UsageError, match=message):
            cli.parse_args(ref + q + flags)
    with pytest.raises(cli.UsageError, match="--format-on-gpu and --out-mutations exclude each other"):   # (without the flag the rule stands)
        cli.parse_args(ref + q + mut + ["--out-sam", "o.sam", "--format-on-gpu"])


class KeepingDatabase(StandInDatabase):
    """The stand-in as a context whose last batch and alignments a pile-up can read."""

    def __init__(self, contigs, *a, **k):
        super().__init__(contigs, *a, **k)
        self.contigs = [(n, api.encode(t) if isinstance(t, str) else np.asarray(t, np.uint8)) for n, t in contigs]

    def align_stream(self, batches, parameters, on_aligned=None):
        p = parameters._c()
        for k, arrays in enumerate(batches):
            batch = oracle_lib.QueryBatch.from_arrays(*arrays)
            s = self.oracle.align(batch, p)
            result = api.BatchResult(dict(ints=s.ints, dbls=s.dbls, int_off=s.int_off, dbl_off=s.dbl_off, extra=[0] * 8))
            self.last = (batch, result)
            if on_aligned is not None:
                on_aligned(k)
            yield result


class ModelMatchDatabase(pileup.CountedMatchDatabase):
    """pileup.MatchDatabase for the command line without a GPU: the plain recount (tests/pileup_model.py) piles up what the stand-in aligned, the host path is
    CountedMatchDatabase's, and the device path is the rules' program over the same counts."""
    program, tmp, calls = None, None, []

    def __init__(self, database, query_end_fraction=0.0, keep_insert_text=False):
        self.db, self.model, self.mates = database, PileupModel(database.contigs, query_end_fraction), []
        self.contigs, self.query_end_fraction, self._L, self._h = database.contigs, float(query_end_fraction), None, []

    def add_last(self, queries=None, replica=0):
        batch, result = self.db.last
        mates = [[m.copy() for m in q] for q in W.mates_of(batch)]   # (the reader's buffers go when the batch is written)
        self.mates.append(mates)
        return self.model.add([result.query_alignments(q) for q in range(batch.nq)], mates)

    def _fed(self):
        m = self.model
        return pileup.CountedMatchDatabase(m.contigs, m.depth, m.alt, m.middle, m.sorted_events(), self.mates, m.f)

    def mutations(self, parameters=None, on_gpu=False):
        ModelMatchDatabase.calls.append(bool(on_gpu))
        fed = self._fed()
        if not on_gpu:
            return fed.mutations(parameters)
        indels = list(fed._indels().items())
        m = self.model
        lengths = [len(c) for _, c in m.contigs]
        snps, verdicts = judged(self.program, os.path.join(self.tmp, "job.txt"), lengths, np.concatenate(m.depth), np.concatenate(m.alt, axis=1), np.concatenate(m.middle),
                                parameters, pileup.indel_candidates(indels))
        return mc.rows_from(fed, snps, indels, verdicts)

    def close(self):
        pass


def test_the_job_with_the_flag_writes_the_host_paths_file(program, tmp_path, monkeypatch):
    from mapper_amd import synth
    ref = synth.synthetic_reference(6_000, seed=0xEC011)
    (tmp_path / "ref.fa").write_text(">chrA\n%s\n>chrB\n%s\n" % (api.decode(ref[:4_000]), api.decode(ref[4_000:])))
    reads = list(synth.synthetic_single_end(ref[:4_000], 160, seed=5, indel_prob=0.5)[0]) + list(synth.synthetic_single_end(ref[4_000:], 80, seed=6, indel_prob=0.5)[0])
    (tmp_path / "se.fq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)) for i, r in enumerate(reads)))
    monkeypatch.setattr(pileup, "MatchDatabase", ModelMatchDatabase)
    ModelMatchDatabase.program, ModelMatchDatabase.tmp = program, str(tmp_path)
    job = ["--reference", str(tmp_path / "ref.fa"), "--queries", str(tmp_path / "se.fq"), "--batch-size", "64", "--contexts", "1"]
    outs = {}
    for thresholds in ([], ["--snp-threshold", "0", "0", "--indel-threshold", "0", "0"], ["--snp-threshold", "2", "0.3", "--indel-threshold", "1.5", "0.35"]):
        for mode, flags in (("host", []), ("gpu", ["--call-mutations-on-gpu"])):
            StandInDatabase.opened.clear()
            del ModelMatchDatabase.calls[:]
            path, log = str(tmp_path / (mode + ".txt")), io.StringIO()
            assert cli.run(job + ["--out-mutations", path] + thresholds + flags, out=log, open_database=KeepingDatabase) == 0
            assert ModelMatchDatabase.calls == [mode == "gpu"] and StandInDatabase.opened[0].closed
            outs[mode] = (open(path, "rb").read(), log.getvalue())
        assert outs["gpu"] == outs["host"]
        body = [l.split(b"\t") for l in outs["host"][0].split(b"\n") if l and not l.startswith(b"#") and not l.startswith(b"CHR")]
        if thresholds and thresholds[1] == "0":   # everything: SNPs, insertions and deletions on both contigs
            assert len(body) > 100 and {l[0] for l in body} == {b"chrA", b"chrB"}
            assert any(set(l[2]) == {ord("-")} for l in body) and any(set(l[3]) == {ord("-")} for l in body)
            everything = len(body)
        elif thresholds:
            assert 0 < len(body) < everything
