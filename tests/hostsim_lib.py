"""Host simulation of the device kernel (tests/hostsim/xm_hostsim.cpp) — TEST HARNESS ONLY, never used by the product."""
import ctypes as C
import os
import subprocess
import numpy as np

from mapper_amd import _capi
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "xm_hostsim.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libxm_hostsim.so")


def build():
    """XMSIM_POISON=1 (read when the library is first loaded): the variant built with -DXM_ARENA_POISON - every arena allocation starts as garbage, so a structure
    that is read before it is written (on the GPU: a result that depends on which read used the lane before) shows up as a difference from the oracle."""
    poison = os.environ.get("XMSIM_POISON") == "1"
    out = OUT.replace(".so", "_poison.so") if poison else OUT
    deps = [SRC] + [os.path.join(ROOT, "mapper_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "mapper_amd", "csrc")) if f.endswith(".h")]
    import fcntl
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out + ".lock", "w") as lock:  # (pytest-xdist workers build side by side)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] +
                                  (["-DXM_ARENA_POISON"] if poison else []) + ["-o", out + ".tmp", SRC])
            os.replace(out + ".tmp", out)
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.xmsim_last_error.restype = C.c_char_p
        L.xmsim_index_build.restype = C.c_void_p
        L.xmsim_index_build.argtypes = [C.POINTER(_capi.XmRef), C.POINTER(_capi.XmBuildOpts)]
        L.xmsim_index_free.argtypes = [C.c_void_p]
        L.xmsim_align_batch.argtypes = [C.c_void_p, C.POINTER(_capi.XmParams), C.POINTER(_capi.XmQueryBatch), C.POINTER(C.POINTER(_capi.XmResult))]
        L.xmsim_result_free.argtypes = [C.POINTER(_capi.XmResult)]
        L.xmsim_table_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.xmsim_table_dump.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.xmsim_index_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.xmsim_ensure_length.argtypes = [C.c_void_p, C.c_int]
        L.xmsim_dup_keys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.xmsim_dup_keys.restype = C.c_int64
        L.xmsim_pyramid_dump.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.xmsim_pyramid_dump.restype = C.c_int64
        L.xmsim_pyramid_dump_multi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        L.xmsim_pyramid_dump_multi.restype = C.c_int64
        L.xmsim_kat_multi_contains.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.xmsim_kat_position_codec.argtypes = [C.c_int, C.c_int]
        L.xmsim_test_bound.argtypes = [C.POINTER(_capi.XmParams), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.xmsim_set_wave_mode.argtypes = [C.c_int]
        L.xmsim_wave_status_counts.argtypes = [C.c_void_p, C.c_int]
        L.xmsim_pass_policy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.xmsim_plan_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        L.xmsim_next_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xmsim_first_arena_size.argtypes = [C.c_int64, C.c_uint64, C.c_int]
        L.xmsim_first_arena_size.restype = C.c_uint64
        L.xmsim_grown_arena_size.argtypes = [C.c_uint64, C.c_uint64]
        L.xmsim_grown_arena_size.restype = C.c_uint64
        L.xmsim_table_shape.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.xmsim_table_shape.restype = None
        L.xmsim_plan_groups.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_int64]
        L.xmsim_plan_groups.restype = C.c_int64
        L.xmsim_layout_group.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.xmsim_layout_group.restype = C.c_int64
        L.xmsim_sort_key_bits.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
        L.xmsim_sort_key_bits.restype = None
        L.xmsim_conf_new.restype = C.c_void_p
        L.xmsim_conf_free.argtypes = [C.c_void_p]
        L.xmsim_conf_prepare.argtypes = [C.c_void_p, C.POINTER(_capi.XmParams), C.c_void_p, C.c_int64, C.c_double, C.c_int64, C.c_int64]
        L.xmsim_conf_prepare.restype = None
        L.xmsim_conf_insert.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xmsim_conf_insert.restype = C.c_int64
        L.xmsim_conf_lookup.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xmsim_conf_lookup.restype = C.c_int64
        L.xmsim_conf_state.argtypes = [C.c_void_p, C.c_void_p]
        L.xmsim_conf_mark_uploaded.argtypes = [C.c_void_p]
        L.xmsim_conf_dump.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xmsim_conf_dump.restype = C.c_int64
        L.xmsim_conf_values.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_void_p]
        L.xmsim_conf_values.restype = None
        _lib = L
    return _lib


def build_opts(mode="mapper", enable_gapmers=True, custom_dup=None, max_hashed_length=0, host_only=0):
    o = _capi.XmBuildOpts()
    o.enable_gapmers = 1 if enable_gapmers else 0
    o.min_interesting_size = -1
    o.max_hashed_length = max_hashed_length
    o.dup_window = 1 if mode == "api" else 1000
    o.dup_min_copies = 2
    o.dup_min_length = o.dup_max_length = -1
    if custom_dup:
        o.dup_min_length, o.dup_max_length, o.dup_min_copies, o.dup_window = custom_dup
    o.device = -1
    o.host_only = host_only
    return o


def _xm_params(params):
    p = _capi.XmParams()
    for f, _ in _capi.XmParams._fields_:
        if f != "reserved":
            setattr(p, f, getattr(params, f))
    return p


class SimReference:
    def __init__(self, contigs, mode="mapper", enable_gapmers=True, custom_dup=None):
        self.L = lib()
        cs = [(n, oracle_lib.encode(s) if isinstance(s, str) else np.ascontiguousarray(s, dtype=np.uint8)) for n, s in contigs]
        ref, self._keep = _capi.make_ref(cs)
        o = build_opts(mode, enable_gapmers, custom_dup)
        self.h = self.L.xmsim_index_build(C.byref(ref), C.byref(o))
        if not self.h:
            raise RuntimeError(self.L.xmsim_last_error().decode())
        self.h = C.c_void_p(self.h)

    def __del__(self):
        try:
            self.L.xmsim_index_free(self.h)
        except Exception:
            pass

    def align(self, batch, params):
        if not isinstance(batch, oracle_lib.QueryBatch):
            batch = oracle_lib.QueryBatch(batch)
        b, keep = _capi.make_batch(batch.mate_count, batch.mate_offset, batch.mate_length, batch.codes, batch.expected_inner, batch.deviation)
        p = _xm_params(params)
        res = C.POINTER(_capi.XmResult)()
        if self.L.xmsim_align_batch(self.h, C.byref(p), C.byref(b), C.byref(res)):
            raise RuntimeError(self.L.xmsim_last_error().decode())
        d = _capi.copy_result(res.contents)
        self.L.xmsim_result_free(res)
        st = oracle_lib.Streams(d["ints"], d["dbls"], d["int_off"], d["dbl_off"], d["counters"])
        st.extra = d["extra"]  # the rejection filter in front of PathAligner: searches taken, rejected, cells, active (include/xmapper_hip.h)
        return st

    def index_info(self):
        a, b = C.c_int32(), C.c_int32()
        self.L.xmsim_index_info(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def ensure_length(self, n):
        if self.L.xmsim_ensure_length(self.h, n):
            raise RuntimeError(self.L.xmsim_last_error().decode())

    def table(self, L_):
        cap, mx, n = C.c_int32(), C.c_int32(), C.c_int64()
        if self.L.xmsim_table_info(self.h, L_, C.byref(cap), C.byref(mx), C.byref(n)):
            return None
        counts = np.zeros(cap.value, dtype=np.int32)
        pos = np.zeros(max(n.value, 1), dtype=np.int64)
        self.L.xmsim_table_dump(self.h, L_, counts.ctypes.data, pos.ctypes.data)
        return dict(capacity=cap.value, maxCount=mx.value, counts=counts, positions=pos[:n.value])

    def dup_keys(self, contig):
        n = self.L.xmsim_dup_keys(self.h, contig, None, 0)
        out = np.zeros(max(n, 1), dtype=np.int32)
        self.L.xmsim_dup_keys(self.h, contig, out.ctypes.data, n)
        return out[:n]


def pyramid_dump(codes):
    L = lib()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    cap = 64 * (len(codes) + 4) + 64
    out = np.zeros((cap, 14), dtype=np.int32)
    n = L.xmsim_pyramid_dump(codes.ctypes.data, len(codes), out.ctypes.data, cap)
    assert 0 <= n <= cap
    return out[:n]


def pyramid_dump_multi(codes, scale=1):
    """the product's read-side pyramid with its multi blocks, pools sized for `scale` as compInit sizes them; None = a capacity was exceeded at that scale"""
    L = lib()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    cap = 4096
    while True:
        out = np.zeros((cap, 12), dtype=np.int32)
        n = L.xmsim_pyramid_dump_multi(codes.ctypes.data, len(codes), scale, out.ctypes.data, cap)
        if n < 0:
            return None
        if n <= cap:
            return out[:n]
        cap = n


def set_wave_mode(mode):
    """0: lane-per-read pass sequence only; 1: the wave-per-read form's light tier first; 2: + its chain tier; 3: + its search tier (what the product runs)."""
    lib().xmsim_set_wave_mode(mode)


def wave_status_counts(reset=True):
    """How the wave form left the reads since the last reset: index = status (0 finished there, 8 left to the lane-per-read passes, 9 handed to the heavy tier)."""
    out = np.zeros(16, dtype=np.int64)
    lib().xmsim_wave_status_counts(out.ctypes.data, 1 if reset else 0)
    return out


def test_bound(params, query, query_rc, start_a, end_a, reference, start_b, end_b, predicted_best_offset=0):
    """the rejection filter of xm_bound.h alone (host-compiled) -> (taken, rejected, cells)"""
    q = np.ascontiguousarray(query, dtype=np.uint8)
    r = np.ascontiguousarray(reference, dtype=np.uint8)
    p = _xm_params(params)
    out = (C.c_int64 * 3)()
    lib().xmsim_test_bound(C.byref(p), q.ctypes.data, len(q), 1 if query_rc else 0, start_a, end_a, r.ctypes.data, len(r), start_b, end_b, predicted_best_offset, out)
    return int(out[0]), int(out[1]), int(out[2])


# ---- the product's pass planner (mapper_amd/csrc/xm_pass_plan.h); the knobs are read from the environment as an align call reads them
POLICY_FIELDS = ("seedScale", "gappedScale", "longReads", "arenaUnit", "lightTmpUnit", "regionBytes", "scratchWanted", "boundFilterOn", "searchPoolOn", "heavyHint", "lightWaves",
                 "fullWaves", "lightLpw", "fullLpw", "gappedTmpBytes", "handOver")
STATE_FIELDS = ("heavy", "hoMode", "scale", "overflowScale", "orderedList", "ts", "to", "tc", "confRounds", "nRegions", "regionsTotal")
PLAN_FIELDS = ("arenaBytes", "lpw", "nWaves", "grid", "block", "lanes", "nRegions", "regionsTotal", "scratchBytes", "gappedReserve", "pairLanes", "boundFilter", "boundFilterArg",
               "firstStride", "firstItem", "poolBuffers", "taperUnit")
PASS_KINDS = ("done", "out_rerun", "gapped", "conf_rerun", "scale_rerun")


def _facts(longest_mate, paired=False, contexts=1, context_scratch=0):
    return np.array([longest_mate, 1 if paired else 0, contexts, context_scratch], dtype=np.int64)


def _check(rc):
    if rc:
        raise RuntimeError(lib().xmsim_last_error().decode())


def pass_policy(longest_mate, paired=False, contexts=1, context_scratch=0):
    """-> (policy dict, state dict of the first pass) of a batch"""
    f, pol, st = _facts(longest_mate, paired, contexts, context_scratch), np.zeros(16, dtype=np.int64), np.zeros(11, dtype=np.int64)
    _check(lib().xmsim_pass_policy(f.ctypes.data, pol.ctypes.data, st.ctypes.data))
    return dict(zip(POLICY_FIELDS, map(int, pol))), dict(zip(STATE_FIELDS, map(int, st)))


def plan_launch(state, n_todo, nq, num_cus, budget, scratch_held, longest_mate, paired=False, contexts=1, context_scratch=0):
    f, plan = _facts(longest_mate, paired, contexts, context_scratch), np.zeros(17, dtype=np.int64)
    st = np.array([state[k] for k in STATE_FIELDS], dtype=np.int64)
    _check(lib().xmsim_plan_launch(f.ctypes.data, st.ctypes.data, n_todo, nq, num_cus, budget, scratch_held, plan.ctypes.data))
    return dict(zip(PLAN_FIELDS, map(int, plan)))


def next_pass(state, ctl, longest_mate, paired=False, contexts=1):
    """ctl: dict with nHeavy, nHeavyLate, nScale (2), nOut (2), nConf (2) (missing = 0) -> (kind, nTodo, list, clear, new state)"""
    f, nxt = _facts(longest_mate, paired, contexts), np.zeros(4, dtype=np.int64)
    st = np.array([state[k] for k in STATE_FIELDS], dtype=np.int64)
    c = np.array([ctl.get("nHeavy", 0), ctl.get("nHeavyLate", 0)] + list(ctl.get("nScale", (0, 0))) + list(ctl.get("nOut", (0, 0))) + [2 ** 64 - 1] + list(ctl.get("nConf", (0, 0))), dtype=np.uint64)
    _check(lib().xmsim_next_pass(f.ctypes.data, st.ctypes.data, c.ctypes.data, nxt.ctypes.data))
    return PASS_KINDS[int(nxt[0])], int(nxt[1]), int(nxt[2]), int(nxt[3]), dict(zip(STATE_FIELDS, map(int, st)))


def first_arena_size(nq, hits=0, doubles=False):
    """elements of a result arena (the ints', or the doubles') a call of nq queries starts with, `hits` of them for the slices a memory replays"""
    return int(lib().xmsim_first_arena_size(nq, hits, 1 if doubles else 0))


def grown_arena_size(cap, cursor):
    """elements a result arena of `cap` grows to after a pass that asked for `cursor`"""
    return int(lib().xmsim_grown_arena_size(cap, cursor))


# ---- the index-build planner (mapper_amd/csrc/xm_index_plan.h), shared by the host builder and the GPU builder
def table_shape(estimated_capacity, L_, max_num_short_matches):
    """-> (capacity, maxCount) of table L_"""
    out = np.zeros(2, dtype=np.int64)
    lib().xmsim_table_shape(estimated_capacity, L_, max_num_short_matches, out.ctypes.data)
    return int(out[0]), int(out[1])


def plan_groups(hist, min_len, budget):
    """hist[L] = records of table L, L = 0 .. len(hist) - 1 -> [(gLo, gHi, nRecs)] of the tables [min_len, len(hist) - 1]"""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    out = np.zeros((len(h) + 1, 3), dtype=np.int64)
    n = lib().xmsim_plan_groups(h.ctypes.data, min_len, len(h) - 1, budget, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    return [tuple(int(v) for v in row) for row in out[:n]]


def layout_group(hist, capacity, max_count, g_lo, g_hi):
    """the planned shapes and the records of the tables 0 .. g_hi -> ([(bucketBase, capacity, maxCount)] of the tables [g_lo, g_hi], nEntries)"""
    h, cap, mx = np.ascontiguousarray(hist, dtype=np.uint64), np.ascontiguousarray(capacity, dtype=np.int32), np.ascontiguousarray(max_count, dtype=np.int32)
    assert len(h) == len(cap) == len(mx) == g_hi + 1
    out = np.zeros((g_hi - g_lo + 1, 3), dtype=np.int64)
    n = lib().xmsim_layout_group(h.ctypes.data, cap.ctypes.data, mx.ctypes.data, g_lo, g_hi, out.ctypes.data)
    return [tuple(int(v) for v in row) for row in out], int(n)


def sort_key_bits(last_cum_start, ambiguous, n_tables):
    """-> (posBits, tableBits) of the GPU build's two radix sorts"""
    out = np.zeros(2, dtype=np.int64)
    lib().xmsim_sort_key_bits(last_cum_start, 1 if ambiguous else 0, n_tables, out.ctypes.data)
    return int(out[0]), int(out[1])


# ---- the host's confidence table (mapper_amd/csrc/xm_conf_table.h)
def _keys(penalties, lens):
    return np.ascontiguousarray(penalties, dtype=np.float64), np.ascontiguousarray(lens, dtype=np.int32)


def conf_values(penalties, lens, params, granularity, total_size):
    """confidenceLengthOnHost (xm_confidence.h) of every key"""
    pen, ln = _keys(penalties, lens)
    out = np.zeros(len(pen), dtype=np.float64)
    lib().xmsim_conf_values(len(pen), pen.ctypes.data, ln.ctypes.data, params.Max_PenaltySpan, params.MutationPenalty, granularity, total_size, out.ctypes.data)
    return out


class SimConfTable:
    """A ConfTable as a context holds it; lookups go through the kernels' confLookup."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.xmsim_conf_new())

    def __del__(self):
        try:
            self.L.xmsim_conf_free(self.h)
        except Exception:
            pass

    def prepare(self, params, lens, granularity, total_size, seed_budget):
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        self.L.xmsim_conf_prepare(self.h, C.byref(_xm_params(params)), ln.ctypes.data, len(ln), granularity, total_size, seed_budget)

    def insert(self, penalties, lens):
        """-> per key: was it added"""
        pen, ln = _keys(penalties, lens)
        added = np.zeros(len(pen), dtype=np.uint8)
        self.L.xmsim_conf_insert(self.h, len(pen), pen.ctypes.data, ln.ctypes.data, added.ctypes.data)
        return added.astype(bool)

    def lookup(self, penalties, lens):
        """-> (per key: found, values)"""
        pen, ln = _keys(penalties, lens)
        found, values = np.zeros(len(pen), dtype=np.uint8), np.zeros(len(pen), dtype=np.float64)
        self.L.xmsim_conf_lookup(self.h, len(pen), pen.ctypes.data, ln.ctypes.data, found.ctypes.data, values.ctypes.data)
        return found.astype(bool), values

    def state(self):
        """-> (slots, entries, dirty)"""
        out = np.zeros(3, dtype=np.int64)
        self.L.xmsim_conf_state(self.h, out.ctypes.data)
        return int(out[0]), int(out[1]), bool(out[2])

    def mark_uploaded(self):
        self.L.xmsim_conf_mark_uploaded(self.h)

    def entries(self):
        """-> (penalties, lengths, values) of every entry"""
        n = self.state()[1]
        pen, ln, val = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
        assert self.L.xmsim_conf_dump(self.h, n, pen.ctypes.data, ln.ctypes.data, val.ctypes.data) == n
        return pen, ln, val
