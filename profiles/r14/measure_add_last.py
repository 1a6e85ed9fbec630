"""xm_pileup_add_last per batch with and without kept text; text bytes per million reads."""
import sys, time, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from mapper_amd import api, pileup, synth

def batch_arrays(reads):
    n, L = reads.shape
    return (np.ones(n, np.int32), (np.arange(2 * n, dtype=np.int64) // 2) * L, np.tile(np.array([L, 0], np.int32), n), np.ascontiguousarray(reads).reshape(-1),
            np.zeros(n), np.ones(n))

def measure(name, ref_len, n_reads, ref_seed, read_seed, indel_prob, reps=7):
    ref = synth.synthetic_reference(ref_len, seed=ref_seed)
    reads = synth.synthetic_single_end(ref, n_reads, seed=read_seed, indel_prob=indel_prob)[0]
    db = api.ReferenceDatabase([("r", ref)])
    res = db.align_arrays(*batch_arrays(reads), api.AlignmentParameters())
    out = {}
    for keep in (False, True, False, True):
        m = pileup.MatchDatabase(db, 0.1, keep_insert_text=keep)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            total = m.add_last(None)
            times.append((time.perf_counter() - t0) * 1e3)
        out.setdefault(keep, []).append(times)
        if keep:
            L, h = m._L, m._h[0]
            per_call = total // reps
            import ctypes as C
            off = np.zeros(per_call + 1, np.int64); text = np.zeros(64 << 20, np.uint8)
            got = L.xm_pileup_event_text(h, 0, per_call, off.ctypes.data, text.ctypes.data, len(text))
            ev = np.zeros((per_call, 8), np.int64); L.xm_pileup_events(h, 0, per_call, ev.ctypes.data)
            text_bytes, n_ins, n_ev = int(off[got]), int((ev[:, 2] == 1).sum()), per_call
            assert got == per_call
        m.close()
    for keep in (False, True):
        runs = out[keep]
        print("%s keep_text=%s add_last ms per call: first %s median-of-rest %s" % (name, keep, ["%.3f" % r[0] for r in runs], ["%.3f" % float(np.median(r[1:])) for r in runs]))
    print("%s events per batch %d, insertions %d, text bytes %d = %.0f bytes per million reads" % (name, n_ev, n_ins, text_bytes, text_bytes * 1e6 / n_reads))
    db.close()

measure("3000 reads / 20 kb (indel_prob 0.3)", 20_000, 3000, 91, 92, 0.3)
measure("configs[1] batch: 1M reads / 5 Mb", 5_000_000, 1_000_000, 0xEC011, 0x5EED0001, 0.05, reps=5)
