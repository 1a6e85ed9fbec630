"""Counts, events and filters for the mutation-calling tests (tests/test_mutations_rules.py without a GPU, tests/test_gpu_mutations.py on one), and the host
answer they are compared with: pileup.CountedMatchDatabase.mutations() - the definition - over the same counts.

TEST INFRASTRUCTURE ONLY.  Counts are flat over all forward positions, as a device pile-up holds them: depth[total], alt[4, total], middle[total], in units of
1 / UNIT; every case is a pure function of its seed."""
import numpy as np

from mapper_amd import _capi, api, pileup

UNIT = pileup.UNIT
Filter = pileup.MutationDetectionParameters
CODES = np.array([1, 2, 4, 8], np.uint8)


def filters():
    """The empty filter, the default one, and one that drops about half of the rows of random_counts() (depths of 1 .. 12 reads, supports of 1 .. depth)."""
    return {"empty": Filter.emptyFilter(), "default": Filter.defaultFilter(), "half": Filter(4.0, 0.5, 1.0, 0.25, 1.0, 0.25)}


def contigs_of(lengths, seed=7):
    rng = np.random.default_rng(seed)
    return [("c%d" % i, CODES[rng.integers(0, 4, n)]) for i, n in enumerate(lengths)]


def split(flat, lengths):
    """A flat array (last axis: all forward positions) -> one array per contig."""
    at = np.concatenate([[0], np.cumsum(lengths)])
    return [np.ascontiguousarray(flat[..., at[c]:at[c + 1]]) for c in range(len(lengths))]


def counted(lengths, depth, alt, middle, events=(), fraction=0.0, seed=7):
    """The host half over flat counts."""
    return pileup.CountedMatchDatabase(contigs_of(lengths, seed), split(depth, lengths), split(alt, lengths), split(middle, lengths), list(events), (), fraction)


def empty_counts(total):
    return np.zeros(total, np.uint64), np.zeros((4, total), np.uint64), np.zeros(total, np.uint64)


def random_counts(total, density, seed, whole_reads=True):
    """Depths of 1 .. 12 reads everywhere; at a share `density` of the (position, letter) pairs an alt of 1 .. depth reads (density 1: every pair, 4 rows a
    position with the empty filter); a middle depth somewhere between 0 and the depth.  whole_reads=False: units that are no multiple of UNIT."""
    rng = np.random.default_rng(seed)
    reads = rng.integers(1, 13, total).astype(np.uint64)
    depth = reads * np.uint64(UNIT)
    if not whole_reads:
        depth = depth - rng.integers(0, UNIT // 2, total).astype(np.uint64)
    alt = np.zeros((4, total), np.uint64)
    mask = rng.random((4, total)) < density
    support = (rng.integers(1, 13, (4, total)).astype(np.uint64) % reads + np.uint64(1)) * np.uint64(UNIT)
    if not whole_reads:
        support = support - rng.integers(0, UNIT // 3, (4, total)).astype(np.uint64)
    alt[mask] = np.minimum(support, depth[None, :])[mask]
    middle = (depth // np.uint64(12)) * rng.integers(0, 13, total).astype(np.uint64)
    return depth, alt, middle


def random_events(lengths, n, seed, flagged=0.0):
    """n insertion / deletion events anywhere on the contigs - at the first and last bases too, deletions that run to and past the end of their contig -, several
    of them at one place so that they group; a share `flagged` near a query end (dropped by the grouping)."""
    rng = np.random.default_rng(seed)
    events = []
    for k in range(n):
        c = int(rng.integers(0, len(lengths)))
        kind = int(rng.integers(1, 3))
        length = int(rng.choice([1, 1, 2, 3, 5, 9]))
        edge = int(rng.integers(0, 4))
        start = 0 if edge == 0 else max(lengths[c] - (1 if kind == 1 else length), 0) if edge == 1 else int(rng.integers(0, lengths[c]))
        if kind == 1 and edge == 1:
            start = lengths[c]   # an insertion behind the last base
        weight = int(rng.choice([UNIT, UNIT, UNIT // 2, UNIT // 17 + 1, 3 * UNIT]))
        event = (c, start, kind, length, k, 4 if rng.random() < flagged else 0, 10, weight)
        events.append(event)
        if rng.random() < 0.3:
            events.append(event[:4] + (k, 0, 10, UNIT))
    return events


def snp_array(rows):
    """[(contig, position, letter, reference code, support units, total units)] -> xm_snp_row records."""
    out = np.zeros(len(rows), _capi.SNP_ROW)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def rows_from(fed, snps, indels, verdicts):
    """What pileup.MatchDatabase._mutations_on_gpu makes of the device's answer, with the reference allele from the stand-in's contigs."""
    return pileup.merged_rows(snps, indels, verdicts, lambda c, p, code: api.decode(fed.contigs[c][1][p:p + 1]))
