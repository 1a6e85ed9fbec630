"""CPU tier: the pairs of tests/pair_geometry.py - the edges of the mate window, of the spacing penalty's steps, of the join of overlapping mates and of the
unpaired fall-back, spacings that are no ordinary numbers - through the host simulation of the device code, in its lane-per-read form and in its
wave-per-read form (xm_wave.h has its own copy of the pairing code), against the oracle bit for bit; that every class reaches what it was built for, read
from the oracle's answer alone; and the queries for which the reference would have thrown (XM_ST_INTERNAL: status 5)."""
import re
import numpy as np
import pytest

import oracle_lib as o
import hostsim_lib as hs
import pair_geometry as pg
from helpers import streams_equal, first_difference, alignments_per_query, compose_batch

WAVE_MODES = {"lanes": 0, "waves": 3}


@pytest.fixture(scope="module")
def refs():
    contigs, _ = pg.reference()
    return o.OracleReference(contigs), hs.SimReference(contigs)


@pytest.fixture(scope="module")
def answers(refs):
    """{class: [(Group without the queries the oracle throws for, those throwers, the oracle's streams)]}, computed once."""
    out = {}
    for name, make in pg.CLASSES.items():
        out[name] = []
        for g in make():
            keep, thrown = pg.split_throwers(refs[0], g)
            out[name].append((keep, thrown, refs[0].align(pg.batch(keep), o.make_params(keep.params))))
    return out


def paired(comps):
    """one component whose alignments all hold two sequences"""
    return len(comps) == 1 and len(comps[0]) >= 1 and all(len(a["sequences"]) == 2 for a in comps[0])


def shape(comps):
    return [len(c) for c in comps]


@pytest.fixture(params=list(WAVE_MODES))
def form(request):
    hs.set_wave_mode(WAVE_MODES[request.param])
    yield request.param
    hs.set_wave_mode(-1)


@pytest.mark.parametrize("name", list(pg.CLASSES))
def test_simulation_equals_the_oracle(name, form, refs, answers):
    for keep, thrown, want in answers[name]:
        assert name == "odd_spacing" or not thrown, thrown
        assert 0 < len(keep.queries) <= 2000
        hs.wave_status_counts()
        got = refs[1].align(pg.batch(keep), o.make_params(keep.params))
        assert streams_equal(got, want), first_difference(got, want, len(keep.queries))
        if form == "waves":   # its own pairing code ran: it finished most pairs itself, and left the overlapping mates to the lane-per-read passes
            st, n = hs.wave_status_counts(), len(keep.queries)
            assert st[0] + st[8] == n and (st[8] > 0.8 * n if name == "joins" else st[0] > 0.5 * n), st


def test_window_edges_pair_on_the_near_side_only(refs, answers):
    """Both sides of both edges, for every setting, both strands and both orders of the candidate lists: the pairs at the edge and one base inside it
    are one component of two sequences, the pair one base outside is not."""
    seen = set()
    for keep, _, want in answers["window_edges"]:
        for q, (edge, setting, reverse, cands, side) in enumerate(keep.tags):
            assert paired(want.query(q)) == (side <= 0), (keep.tags[q], shape(want.query(q)))
            seen.add((edge, setting, reverse, cands, side))
    assert len(seen) == 2 * len(pg.WINDOW_SETTINGS) * 2 * 3 * 3
    # the product inside (int) is an integer for one setting and not for the others
    whole = [float((a + b) * r * d + e).is_integer() for a, b, r, e, d in pg.WINDOW_SETTINGS]
    assert any(whole) and not all(whole)
    assert any(a != b and a % 2 for a, b, *_ in pg.WINDOW_SETTINGS)


def test_both_orders_of_the_candidate_lists_occur(refs, answers):
    """lastComponentIsLargest: the family mate alone has several alignments and its partner one, once as mate 1 and once as mate 2 - and the lower edge then
    lies at half the length of the mate with more candidates, which the settings with mates of different lengths tell apart."""
    family_mates, partners = [], []
    for keep, _, _ in answers["window_edges"]:
        for (mates, _, _), (edge, setting, reverse, cands, side) in zip(keep.queries, keep.tags):
            if cands != "unique" and side == 0:
                m = 0 if cands == "family1" else 1
                family_mates.append(([mates[m]], 0.0, 1.0))
                partners.append(([mates[1 - m]], 0.0, 1.0))
    assert len(family_mates) == len(pg.WINDOW_SETTINGS) * 2 * 2 * 2
    many = alignments_per_query(refs[0].align(o.QueryBatch(family_mates), o.make_params(MaxErrorRate=0.07)))
    one = alignments_per_query(refs[0].align(o.QueryBatch(partners), o.make_params(MaxErrorRate=0.07)))
    assert (many > 1).all() and (one == 1).all(), (many, one)
    assert any(a // 2 != b // 2 for a, b, *_ in pg.WINDOW_SETTINGS)


def test_spacing_steps_cost_what_the_rule_says(answers):
    (keep, _, want), = answers["spacing_steps"]
    penalties, strands, zero_zone = set(), set(), set()
    for q, (_, setting, inner, reverse, penalty) in enumerate(keep.tags):
        len1, len2 = pg.STEP_SETTINGS[setting][:2]
        comps = want.query(q)
        assert paired(comps) == (penalty <= int((len1 + len2) * 0.1)), (keep.tags[q], shape(comps))
        if paired(comps):
            assert [a["spacingPenalty"] for a in comps[0]] == [float(penalty)], keep.tags[q]
            penalties.add(penalty)
            strands.add(reverse)
            if inner in (-1, 0, 1):
                zero_zone.add((setting, inner, penalty > 0))
    assert penalties >= {0, 1, 2, 3, 4} and strands == {False, True}
    assert {(0, -1, False), (0, 0, True), (0, 1, True)} <= zero_zone, zero_zone


def overlap_on_the_reference(al):
    a, b = ([(blk[1], blk[1] + blk[3]) for blk in s["blocks"]] for s in al["sequences"])
    return min(a[-1][1], b[-1][1]) - max(a[0][0], b[0][0])


def test_joins_occur_and_so_do_unjoinable_mates(answers):
    (keep, _, want), = answers["joins"]
    joined, unjoinable, contained = set(), set(), set()
    for q, (what, overlap, kind, reverse, agree) in enumerate(keep.tags):
        comps = want.query(q)
        if what == "contained":
            contained.add((overlap, kind, reverse, paired(comps)))
            continue
        assert paired(comps), (keep.tags[q], shape(comps))
        if kind in ("exact", "shorter"):
            assert agree and overlap_on_the_reference(comps[0][0]) == overlap, keep.tags[q]
            joined.add((overlap, reverse, kind))
        elif kind == "substitution":
            assert not agree and overlap_on_the_reference(comps[0][0]) == overlap, keep.tags[q]
            unjoinable.add((overlap, reverse))
        else:
            assert not agree and overlap_on_the_reference(comps[0][0]) > 0, keep.tags[q]
            unjoinable.add((kind, reverse))
    for reverse in (False, True):
        assert {(n, reverse, "exact") for n in (1, 2, 149, 150)} <= joined and any(k == "shorter" and r == reverse for _, r, k in joined)
        assert {(2, reverse), (60, reverse), ("indel1", reverse), ("indel2", reverse)} <= unjoinable
    assert sum(1 for c in contained if c[3]) >= 4, contained   # (a mate flush with its partner's end is paired, not thrown for)


def test_orientations_and_contig_ends(answers):
    (keep, _, want), = answers["orientation_and_contigs"]
    shapes = {}
    for q, tag in enumerate(keep.tags):
        shapes.setdefault(tag[0], set()).add((paired(want.query(q)), tuple(shape(want.query(q)))))
    assert shapes["FR"] == {(True, (1,))} and shapes["own reverse complement"] == {(True, (1,))}
    for kind in ("FF", "RR", "RF", "two contigs", "identical"):
        assert shapes[kind] == {(False, (0, 0))}, (kind, shapes[kind])
    assert shapes["over the start"] == {(True, (1,))} and shapes["over the end"] == {(True, (1,))}
    assert shapes["both ends"] == {(False, (1, 1))}


def test_fallback_cut_from_both_sides(answers):
    (keep, _, want), = answers["fallback_edges"]
    seen = set()
    for q, (_, which, contig, length, side) in enumerate(keep.tags):
        assert tuple(shape(want.query(q))) == (which if side <= 0 else (0, 0)), (keep.tags[q], shape(want.query(q)))
        seen.add((which, length, side))
    assert seen == {(w, n, s) for w in ((1, 0), (0, 1)) for n in pg.FALLBACK_LENGTHS for s in (-1, 0, 1)}
    assert [pg.fallback_cut(150, 0.1, d) for _, d in pg.FALLBACK_SETTINGS] == [750, 115]   # (FALLBACK_DISTANCES of the pile-up workloads stop at 700)


def test_odd_spacings_align_or_throw_alike(refs, answers, form):
    """Every odd value aligns on at least one strand; where the oracle throws for one, so does the simulation, and for nothing else."""
    (keep, thrown, _), = answers["odd_spacing"]
    aligned = {(e if e == e else "nan", d if d == d else "nan") for _, e, d, _ in keep.tags}
    for d in pg.ODD_DEVIATIONS:
        assert (pg.SPACING[0], d if d == d else "nan") in aligned
    for e in pg.ODD_EXPECTED:
        assert (e if e == e else "nan", pg.SPACING[1]) in aligned
    assert {r for _, _, _, r in keep.tags} == {False, True}
    assert thrown and all(text.endswith(pg.WRAPPED_WINDOW) for _, _, text in thrown), thrown
    for tag, q, _ in thrown:
        with pytest.raises(RuntimeError, match=r"Failed to align query 0 \((wave )?status 5\)"):
            refs[1].align(o.QueryBatch([q]), o.make_params())


def test_every_thrower_throws(refs, form):
    thrown = pg.throwers()
    kinds = {k for k in pg.THROWER_KINDS for kind, _, _ in thrown if kind.startswith(k)}
    assert kinds == set(pg.THROWER_KINDS)
    names = [kind for kind, _, _ in thrown]
    for must in ("mate 2 in mate 1", "mate 1 in mate 2", "0 bases in", "forward strand", "reverse strand", "deviation 72000000.0", "deviation 1000000000000.0", "deviation inf"):
        assert any(must in n for n in names), must
    for kind, q, text in thrown:
        with pytest.raises(RuntimeError, match=re.escape(text)):
            refs[0].align(o.QueryBatch([q]), o.make_params())
        with pytest.raises(RuntimeError, match=r"Failed to align query 0 \((wave )?status 5\)"):
            refs[1].align(o.QueryBatch([q]), o.make_params())


def test_a_mixed_batch_fails_and_its_other_queries_align(refs, form):
    """Throwers among ordinary queries: both sides fail the batch, the simulation names a thrower, and every other query aligns alone - to the same streams
    as the batch without the throwers."""
    ordinary = pg.ordinary_queries(60)
    thrown = pg.throwers()
    at = [3 + 4 * k for k in range(len(thrown))]
    mixed = pg.with_throwers(ordinary, [(i, q) for i, (_, q, _) in zip(at, thrown)])
    b = o.QueryBatch(mixed)
    with pytest.raises(RuntimeError):
        refs[0].align(b, o.make_params())
    with pytest.raises(RuntimeError, match=r"status 5") as err:
        refs[1].align(b, o.make_params())
    assert int(re.search(r"query (\d+)", str(err.value)).group(1)) in at
    rest = [i for i in range(len(mixed)) if i not in at]
    want = refs[0].align(compose_batch(b, rest), o.make_params())
    got = refs[1].align(compose_batch(b, rest), o.make_params())
    assert streams_equal(got, want), first_difference(got, want, len(rest))
    for j, i in enumerate(rest):
        one = refs[0].align(compose_batch(b, [i]), o.make_params())
        assert np.array_equal(one.ints, want.ints[want.int_off[j]:want.int_off[j + 1]]), i
