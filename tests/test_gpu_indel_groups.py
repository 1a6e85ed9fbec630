"""The pile-up's indel events grouped on the device (xm_pileup_group_events, xm_pileup_call_indels, the fold of xm_pileup_absorb) against the
definition, the host's grouping of the same events (pileup.MatchDatabase._indels()): synthetic events through xm_test_pileup_group - on the edges of the
wavefront and of the scan's block, one key and all keys distinct, long letters, growth from four slots, fingerprints of two bits, absorbed sets -, real
alignments added to a plain and to a grouping pile-up, two contexts whose pile-ups are absorbed, the command line with and without --group-indels-on-gpu, and
the contract of the entries.  Every comparison is equality of group dicts, of row lists or of file bytes."""
import ctypes as C
import io

import numpy as np
import pytest

import indel_groups_cases as gc
import mutations_cases as mc
import oracle_lib
import pileup_workloads as W
from mapper_amd import _capi, api, cli, multi, pileup, synth

UNIT = gc.UNIT
FILTERS = mc.filters()


def device_fold(sets, bits=64, capacity=1 << 12):
    """xm_test_pileup_group over one or two sets of calls -> ({key: units} of set 0's groups, [(call, event, letters)] left over, the growths, the figures)."""
    L = _capi.lib()
    keep = []
    job = _capi.XmTestGroupJob()
    job.fingerprint_bits, job.initial_capacity = bits, capacity
    events_in_all = letters_in_all = 0
    for s, calls in enumerate(sets):
        arr = (_capi.XmTestGroupCall * max(len(calls), 1))()
        for k, call in enumerate(calls):
            ev = np.ascontiguousarray(np.array([e for e, _ in call], np.int64).reshape(-1, 8))
            texts = [t.encode("ascii") for _, t in call]
            off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
            text = np.frombuffer(b"".join(texts) + b"\0", np.uint8).copy()
            keep += [ev, off, text]
            arr[k] = _capi.XmTestGroupCall(len(call), ev.ctypes.data, off.ctypes.data, text.ctypes.data)
            events_in_all, letters_in_all = events_in_all + len(call), letters_in_all + int(off[-1])
        keep.append(arr)
        job.num_calls[s] = len(calls)
        job.calls[s] = C.cast(arr, C.POINTER(_capi.XmTestGroupCall))
    left_events = np.zeros((events_in_all + 1, 8), np.int64)
    left_call = np.zeros(events_in_all + 1, np.int32)
    left_off = np.zeros(events_in_all + 2, np.int64)
    left_text = np.zeros(letters_in_all + 1, np.uint8)
    job.left_cap, job.left_text_cap = events_in_all, letters_in_all
    job.left_events, job.left_call, job.left_text_off, job.left_text = left_events.ctypes.data, left_call.ctypes.data, left_off.ctypes.data, left_text.ctypes.data
    calls = C.POINTER(_capi.XmIndelCalls)()
    if L.xm_test_pileup_group(0, C.byref(job), C.byref(calls)):
        raise RuntimeError(L.xm_last_error().decode())
    try:
        rows, letters, figures = _capi.indel_calls(calls)
    finally:
        L.xm_indel_calls_free(calls)
    groups = {}
    for r in rows:
        assert r["keep"] == r["length"] and r["total_units"] == 0   # (unjudged, and there are no counts)
        key = gc.group_key(int(r["contig"]), int(r["kind"]), int(r["pos1"]), int(r["length"]), letters[r["letters_at"]:r["letters_at"] + r["num_letters"]].decode("ascii"))
        assert key not in groups, key   # a key has one group
        groups[key] = int(r["support_units"])
    n = int(job.num_left)
    assert figures["groups"] == len(rows) and figures["left_over"] == n
    left = [(int(left_call[i]), tuple(int(x) for x in left_events[i]), left_text[left_off[i]:left_off[i + 1]].tobytes().decode("ascii")) for i in range(n)]
    return groups, left, tuple(job.grows), figures


def union(groups, left):
    """The device's groups and the host's groups of the left-overs -> the sum of both (disjoint: whether they must be is the caller's to assert)."""
    out = dict(groups)
    for key, w in gc.definition([[(e, text) for _, e, text in left]]).items():
        out[key] = out.get(key, 0) + w
    return out


def check(calls, **knobs):
    groups, left, grows, figures = device_fold([calls], **knobs)
    host = gc.definition([[(e, text) for _, e, text in left]])
    assert not set(host) & set(groups)   # one pile-up: what the host groups and what the device groups are disjoint
    assert union(groups, left) == gc.definition(calls)
    return groups, left, grows, figures


# ---------------------------------------------------------------- 1. synthetic events
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_event_counts_on_the_wavefront_and_scan_block_edges(n):
    calls = gc.random_calls(n, seed=100 + n, flagged=0.2) if n else [[]]
    groups, left, _, _ = check(calls)
    assert not left and (len(groups) > 0) == (n > 0)
    if n >= 63:
        assert 5 < len(groups) < n   # keys repeat, and not all of them


@pytest.mark.gpu
def test_all_events_on_one_key_and_all_keys_distinct():
    rng = np.random.default_rng(5)
    weights = [int(w) for w in rng.choice([UNIT, UNIT // 2, UNIT // 17 + 1, 3 * UNIT], 4097)]
    groups, left, _, _ = check([[gc.insertion(2, 40, "ACGTTGCA", w, query=k) for k, w in enumerate(weights)]])
    assert not left and groups == {(2, 40, 1, "-" * 8, "ACGTTGCA"): sum(weights)}   # (one slot, 64 lanes of every wavefront adding)
    groups, left, _, _ = check(gc.distinct_calls(4097))
    assert not left and len(groups) == 4097 and set(groups.values()) == {UNIT}


@pytest.mark.gpu
def test_insertion_lengths_around_the_pieces_and_pairs_that_differ_in_the_last_letter():
    rng = np.random.default_rng(9)
    call = []
    for n in (1, 15, 16, 17, 1000):
        stem = gc.random_letters(rng, n - 1)
        for last, weight in (("A", UNIT), ("C", UNIT // 2), ("A", 3 * UNIT)):
            call.append(gc.insertion(0, 50, stem + last, weight))
        call.append(gc.insertion(0, 50, stem + "AG"))   # (and one that differs in length only)
    rng.shuffle(call)
    groups, left, _, _ = check([[(tuple(int(x) for x in e), str(t)) for e, t in call]])
    assert not left and len(groups) == 15
    assert sorted(w for k, w in groups.items() if len(k[4]) == 1000) == [UNIT // 2, 4 * UNIT]


@pytest.mark.gpu
def test_three_calls_that_repeat_keys_of_earlier_calls():
    calls = gc.random_calls(900, seed=21, num_calls=3, places=60, flagged=0.15)
    firsts = [set(gc.definition([c])) for c in calls]
    assert len(firsts[0] & firsts[1]) > 20 and len(firsts[1] & firsts[2]) > 20 and len(firsts[2] - firsts[0] - firsts[1]) > 0
    groups, left, _, _ = check(calls)
    assert not left and len(groups) == len(firsts[0] | firsts[1] | firsts[2])


@pytest.mark.gpu
def test_from_four_slots_the_table_the_records_and_the_arena_grow_several_times():
    calls = gc.distinct_calls(1400, num_calls=7)
    rng = np.random.default_rng(4)
    for k, call in enumerate(calls):
        call += [gc.insertion(2, 10 + k, gc.random_letters(rng, 1 + 300 * k + j)) for j in range(3)]   # (longer letters with every call: the arena grows)
    groups, left, grows, figures = check(calls, capacity=4)
    assert not left and len(groups) == 1400 + 21
    assert all(g >= 2 for g in grows), grows


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_fingerprints_of_two_bits_leave_most_to_the_host_and_whole_ones_nothing(seed):
    calls = gc.random_calls(600, seed=seed, num_calls=3, flagged=0.1, lengths=(1, 2, 17, 40))
    groups, left, _, _ = check(calls, bits=2)
    assert len(left) > 0 and 0 < len(groups) <= 4 and {c for c, _, _ in left} == {0, 1, 2}
    whole, none, _, _ = check(calls, bits=64)
    assert not none and whole == gc.definition(calls) and len(whole) > 100


@pytest.mark.gpu
def test_a_share_of_flagged_events():
    calls = gc.random_calls(2000, seed=33, num_calls=2, flagged=0.5)
    groups, left, _, _ = check(calls)
    everything = gc.definition([[(e[:5] + (e[5] & 3,) + e[6:], t) for e, t in call] for call in calls])
    assert not left and 0 < len(groups) < len(everything) and sum(groups.values()) < sum(everything.values())


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 2])
def test_a_second_set_that_shares_half_its_keys_is_absorbed(bits):
    first = gc.random_calls(800, seed=41, num_calls=2, places=80)
    shared = gc.random_calls(400, seed=41, num_calls=1, places=80)            # (the same seed: the same places and letters)
    own = [[gc.deletion(2, 60 + k % 20, 7 + k // 20, query=k) for k in range(300)]]
    second = [own[0], shared[0]]   # (its own keys first: with few bits they take the slots, and the absorb meets other keys under the same fingerprints)
    keys = (set(gc.definition(first)), set(gc.definition(second)))
    assert len(keys[0] & keys[1]) > 50 and len(keys[1] - keys[0]) > 100 and len(keys[0] - keys[1]) > 0
    groups, left, _, figures = device_fold([first, second], bits=bits, capacity=64)
    assert union(groups, left) == gc.definition(first + second)
    if bits == 64:
        assert not left
    else:   # what the absorb leaves over arrives as events of its own, behind the calls of both sets
        assert any(c == 4 and e[4] == -1 for c, e, _ in left) and len(groups) <= 4


# ---------------------------------------------------------------- 2. real alignments: a plain and a grouping pile-up of one context
def align(db, b):
    return db.align_arrays(b.mate_count, b.mate_offset, b.mate_length, b.codes, b.expected_inner, b.deviation, api.AlignmentParameters())


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["overlapping_pairs", "three_batches", "several_contigs", "fallback_pairs"])
def test_real_alignments_grouped_on_the_device_and_by_the_host(workload):
    contigs, batches = getattr(W, workload)()
    db = api.ReferenceDatabase(contigs)
    for fraction in (0.0, 0.1):
        plain = pileup.MatchDatabase(db, fraction, keep_insert_text=True)
        grouped = pileup.MatchDatabase(db, fraction, keep_insert_text=True, group_on_gpu=True)
        for b in batches:
            align(db, b)
            held = plain.add_last()
            assert grouped.add_last() == 0   # (no left-overs: the host holds no event)
        events = plain._events()
        assert held == len(events) > 50
        assert sum(1 for e in events if e[3] == 1) > 10 and sum(1 for e in events if e[3] == 2) > 10 and (sum(1 for e in events if e[6] & 4) > 0) == (fraction > 0)
        assert any((e[6] >> 1) & 1 for e in events) and (workload not in ("overlapping_pairs", "fallback_pairs") or any(e[6] & 1 for e in events))   # reversed reads, second mates
        assert grouped._L.xm_pileup_events(grouped._h[0], 0, 1, np.zeros(8, np.int64).ctypes.data) == 0 and grouped._events() == []
        want = plain._indels()
        assert grouped._indels() == want and len(want) > 20
        for f in FILTERS.values():
            host = plain.mutations(f)
            assert grouped.mutations(f) == host
            assert grouped.mutations(f, on_gpu=True) == host == plain.mutations(f, on_gpu=True)
            fig = grouped.last_on_gpu
            assert fig["groups"] == len(want) and fig["left_over"] == 0 and fig["candidates"] == 0 and 0 <= fig["kept"] <= fig["groups"]
            assert fig["kept"] == sum(1 for r in host if "-" in r[2] + r[3])   # a row per kept group, and nothing else came down:
            assert 16 + 64 * fig["kept"] <= fig["group_bytes_to_host"] <= 16 + 64 * fig["kept"] + sum(len(k[4]) for k in want if k[2] == 1)
        plain.close(); grouped.close()
    db.close()


@pytest.mark.gpu
def test_two_contexts_of_one_gpu_absorbed_give_the_host_paths_rows():
    ref = synth.synthetic_reference(30_000, seed=61)
    contigs = [("a", ref[:18_000]), ("b", ref[18_000:])]
    reads = list(synth.synthetic_single_end(ref[:18_000], 1200, seed=62, indel_prob=0.4)[0]) + list(synth.synthetic_single_end(ref[18_000:], 800, seed=63, indel_prob=0.4)[0])
    order = np.random.default_rng(64).permutation(len(reads))
    batches = [oracle_lib.QueryBatch([W.single(reads[i]) for i in order[k::4]]) for k in range(4)]
    two = multi.MultiGpuDatabase(contigs, [0, 0])
    plain = pileup.MatchDatabase(two.replicas, 0.1, keep_insert_text=True)
    grouped = pileup.MatchDatabase(two.replicas, 0.1, group_on_gpu=True)
    for k, b in enumerate(batches):
        align(two.replicas[k & 1], b)
        plain.add_last(replica=k & 1)
        grouped.add_last(replica=k & 1)
    want_groups = plain._indels()
    assert grouped._indels() == want_groups and len(want_groups) > 100
    sizes = []
    for f in (mc.Filter(3.0, 0.05, 1.0, 0.05, 1.0, 0.05), mc.Filter.emptyFilter(), mc.Filter.defaultFilter()):
        want = plain.mutations(f)
        assert grouped.mutations(f) == want and grouped.mutations(f, on_gpu=True) == want
        assert grouped.mutations(f) == want and grouped._indels() == want_groups   # (the groups moved into the first pile-up: their sums stay)
        sizes.append(grouped.last_on_gpu["kept"])
    rows, _, figures = grouped._device_groups(grouped._h[1])
    assert len(rows) == 0 and figures["groups"] == 0 and grouped.last_on_gpu["groups"] == len(want_groups)
    # (the empty filter keeps every group; the default one - four fifths of the middle depth - drops the lone indels of a depth of ten)
    assert sizes[1] == len(want_groups) >= sizes[0] >= sizes[2] and sizes[2] < sizes[1]
    plain.close(); grouped.close(); two.close()


# ---------------------------------------------------------------- 3. the command line
def run_job(tmp, tag, extra, batch_size):
    paths = {k: str(tmp / ("%s.%s" % (tag, k))) for k in ("mut", "sam")}
    out = io.StringIO()
    argv = ["--reference", str(tmp / "ref.fasta"), "--queries", str(tmp / "reads.fastq"), "--out-mutations", paths["mut"], "--snp-threshold", "2", "0.05", "--indel-threshold", "1", "0.05",
            "--batch-size", str(batch_size), "--out-sam", paths["sam"]] + extra
    assert cli.run(argv, out=out) == 0
    return {k: open(p, "rb").read() for k, p in paths.items()}, out.getvalue()


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("group_indels_job")
    ref = synth.synthetic_reference(40_000, seed=71)
    reads = list(synth.synthetic_single_end(ref[:25_000], 600, seed=72, indel_prob=0.4)[0]) + list(synth.synthetic_single_end(ref[25_000:], 300, seed=73, indel_prob=0.4)[0])
    with open(tmp / "ref.fasta", "w") as f:
        f.write(">chrA\n" + api.decode(ref[:25_000]) + "\n>chrB\n" + api.decode(ref[25_000:]) + "\n")
    with open(tmp / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, api.decode(r), "I" * len(r)))
    return tmp, {size: run_job(tmp, "host%d" % size, [], size) for size in (1_000_000, 300)}


@pytest.mark.gpu
@pytest.mark.parametrize("batch_size", [1_000_000, 300], ids=["one_batch", "three_batches"])
@pytest.mark.parametrize("name,extra", [("alone", []), ("beside_call", ["--call-mutations-on-gpu"]),
                                        ("beside_all", ["--call-mutations-on-gpu", "--parse-on-gpu", "--format-on-gpu", "--results-on-gpu"])])
def test_cli_writes_the_same_files_with_the_flag(job, name, extra, batch_size):
    tmp, wants = job
    want_files, want_stats = wants[batch_size]
    body = [l.split(b"\t") for l in want_files["mut"].split(b"\n") if l and not l.startswith(b"#") and not l.startswith(b"CHR")]
    assert len(body) > 100 and {l[0] for l in body} == {b"chrA", b"chrB"} and any(set(l[2]) == {ord("-")} for l in body) and any(set(l[3]) == {ord("-")} for l in body)
    assert want_files["mut"] == wants[1_000_000][0]["mut"] and want_files["sam"].count(b"\n") > 900 and "Alignment rate" in want_stats
    files, stats = run_job(tmp, "%s%d" % (name, batch_size), extra + ["--group-indels-on-gpu"], batch_size)
    assert files["mut"] == want_files["mut"] and files["sam"] == want_files["sam"] and stats == want_stats


# ---------------------------------------------------------------- 4. the contract of the entries
@pytest.mark.gpu
def test_the_entries_refuse_what_they_cannot_do():
    ref = synth.synthetic_reference(6_000, seed=5)
    contigs = [("long", ref), ("short", synth.synthetic_reference(2_000, seed=6))]
    b = oracle_lib.QueryBatch(W.noisy_reads(ref, 64, 7))
    db = api.ReferenceDatabase(contigs)
    plain, grouped, late = pileup.MatchDatabase(db, 0.1, keep_insert_text=True), pileup.MatchDatabase(db, 0.1, group_on_gpu=True), pileup.MatchDatabase(db, 0.1)
    L = plain._L
    filt = _capi.XmMutationFilter(0, 0, 0, 0, 0, 0, 0)
    calls = C.POINTER(_capi.XmIndelCalls)()
    assert L.xm_pileup_group_events(None, 1) != 0 and b"null argument" in L.xm_last_error()
    for p, out in ((None, C.byref(calls)), (grouped._h[0], None)):
        assert L.xm_pileup_call_indels(p, C.byref(filt), out) != 0 and b"null argument" in L.xm_last_error()
    assert L.xm_pileup_call_indels(plain._h[0], C.byref(filt), C.byref(calls)) != 0 and b"does not group its events" in L.xm_last_error()
    L.xm_indel_calls_free(None)
    assert L.xm_test_pileup_group(0, None, C.byref(calls)) != 0 and b"null argument" in L.xm_last_error()
    # an empty grouping pile-up: no rows, no buffers, nothing pinned that was not pinned before
    pinned = _capi.pinned_host_bytes()[0]
    assert L.xm_pileup_call_indels(grouped._h[0], None, C.byref(calls)) == 0
    assert calls.contents.num_rows == 0 and not calls.contents.rows and not calls.contents.letters and calls.contents.groups == 0
    L.xm_indel_calls_free(calls)
    assert grouped.mutations(on_gpu=True) == [] == grouped.mutations() and _capi.pinned_host_bytes()[0] == pinned
    align(db, b)
    with pytest.raises(RuntimeError, match="add_last\\(queries\\) with group_on_gpu"):
        grouped.add_last(W.mates_of(b))
    plain.add_last(); grouped.add_last(); late.add_last()
    assert L.xm_pileup_group_events(late._h[0], 1) != 0 and b"alignments were already added" in L.xm_last_error()
    for into, source in ((plain._h[0], grouped._h[0]), (grouped._h[0], plain._h[0])):
        assert L.xm_pileup_absorb(into, source) != 0 and b"groups its events on the device" in L.xm_last_error()
    want = plain.mutations()
    assert len(want) > 20 and grouped.mutations() == want   # (a refused call moved nothing)
    # the pile-up outlives its context, and the buffers come from the pool and go back to it
    db.close()
    assert grouped.mutations(on_gpu=True) == want
    held = _capi.pinned_host_bytes()[0]
    assert grouped.mutations(on_gpu=True) == want and grouped._indels() == plain._indels() and _capi.pinned_host_bytes()[0] == held
    for m in (plain, grouped, late):
        m.close()
