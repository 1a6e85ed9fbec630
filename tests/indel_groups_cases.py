"""Events, calls and the definition for the tests of the indel grouping (tests/test_indel_groups_rules.py without a GPU, tests/test_gpu_indel_groups.py on
one): pileup.CountedMatchDatabase._indels() - the definition - over the events of all calls, with the insertions' letters filed as the device pile-up's kept
text is (_texts).

TEST INFRASTRUCTURE ONLY.  A call is a list of (event, letters): the event the eight fields of xm_pileup_events, the letters a str ('' for a deletion); every
case is a pure function of its seed."""
import numpy as np

import mutations_cases as mc
from mapper_amd import api, pileup

UNIT = pileup.UNIT
LENGTHS = [300, 1, 90]
LETTERS = "ACGT"


def contigs():
    return mc.contigs_of(LENGTHS, seed=17)


def insertion(contig, pos, letters, weight=UNIT, flags=0, query=0):
    return ((contig, pos, 1, len(letters), query, flags, 10, weight), letters)


def deletion(contig, pos, length, weight=UNIT, flags=0, query=0):
    return ((contig, pos, 2, length, query, flags, 10, weight), "")


def definition(calls):
    """{key of _indels(): units} over the events of all calls, by the host's own grouping."""
    events = [e for call in calls for e, _ in call]
    cs = contigs()
    zeros = [np.zeros(len(c), np.uint64) for _, c in cs]
    fed = pileup.CountedMatchDatabase(cs, zeros, [np.zeros((4, len(z)), np.uint64) for z in zeros], zeros, events)
    fed._events = lambda: [(0,) + tuple(int(x) for x in e) for e in events]   # (_events() of a device pile-up files the texts as it pages; here they are filed below)
    fed._texts = {(0, k): text for k, (e, text) in enumerate((e, t) for call in calls for e, t in call) if e[2] == 1}
    return fed._indels()


def group_key(contig, kind, pos1, length, letters):
    """The key of _indels() for a group of the device: (contig, pos1, kind, length, letters)."""
    if kind == 1:
        return (contig, pos1, 1, "-" * length, letters)
    ref = contigs()[contig][1]
    return (contig, pos1, 2, api.decode(ref[pos1 - 1:pos1 - 1 + length]), "-" * length)


def random_letters(rng, n):
    return "".join(LETTERS[i] for i in rng.integers(0, 4, n))


def random_calls(n, seed, num_calls=1, places=None, flagged=0.0, lengths=(1, 2, 3, 5)):
    """n events dealt over num_calls calls, on `places` distinct positions (None: about n / 3, so that keys repeat within and across calls), insertions and
    deletions mixed, weights that are no whole reads among them, a share `flagged` near a query end."""
    rng = np.random.default_rng(seed)
    places = places or max(n // 3, 1)
    spots = [(int(c), int(rng.integers(0, LENGTHS[c]))) for c in rng.integers(0, len(LENGTHS), places)]
    texts = [[random_letters(rng, int(rng.choice(lengths))) for _ in range(2)] for _ in spots]
    calls = [[] for _ in range(num_calls)]
    for k in range(n):
        s = int(rng.integers(0, places))
        c, pos = spots[s]
        weight = int(rng.choice([UNIT, UNIT, UNIT // 2, UNIT // 17 + 1, 3 * UNIT]))
        flags = (4 if rng.random() < flagged else 0) | int(rng.integers(0, 4))
        if rng.random() < 0.5:
            item = insertion(c, pos, texts[s][int(rng.integers(0, 2))], weight, flags, k)
        else:
            item = deletion(c, pos, int(rng.choice(lengths)), weight, flags, k)
        calls[k * num_calls // n].append(item)
    return calls


def distinct_calls(n, num_calls=1):
    """n events with n distinct keys: deletions of growing lengths on a few positions."""
    calls = [[] for _ in range(num_calls)]
    for k in range(n):
        calls[k * num_calls // n].append(deletion(0 if k % 2 == 0 else 2, k % 7, 1 + k // 14, query=k))   # (k mod 14 and k div 14 name k)
    assert len(set(e[:4] for call in calls for e, _ in call)) == n
    return calls
