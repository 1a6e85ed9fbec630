"""ctypes binding of libxmapper_hip.so (include/xmapper_hip.h).  No CPU fallback: if the HIP library cannot be loaded
the import of this module fails loudly."""
import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "_lib", "libxmapper_hip.so")


class XmParams(C.Structure):
    """xm_params = AlignmentParameters (M/AlignmentParameters.java:8-35)."""
    _fields_ = [("MutationPenalty", C.c_double), ("InsertionStart_Penalty", C.c_double), ("InsertionExtension_Penalty", C.c_double),
                ("DeletionStart_Penalty", C.c_double), ("DeletionExtension_Penalty", C.c_double), ("MaxErrorRate", C.c_double),
                ("UnalignedPenalty", C.c_double), ("AmbiguityPenalty", C.c_double), ("Max_PenaltySpan", C.c_double),
                ("MaxNumMatches", C.c_int32), ("reserved", C.c_int32)]


class XmRef(C.Structure):
    _fields_ = [("num_contigs", C.c_int32), ("names", C.POINTER(C.c_char_p)), ("codes", C.POINTER(C.c_void_p)), ("lengths", C.POINTER(C.c_int64))]


class XmBuildOpts(C.Structure):
    _fields_ = [("enable_gapmers", C.c_int32), ("min_interesting_size", C.c_int32), ("max_hashed_length", C.c_int32), ("dup_window", C.c_int32),
                ("dup_min_copies", C.c_int32), ("dup_min_length", C.c_int32), ("dup_max_length", C.c_int32), ("device", C.c_int32),
                ("host_only", C.c_int32), ("reserved", C.c_int32)]


class XmQueryBatch(C.Structure):
    _fields_ = [("num_queries", C.c_int64), ("mate_count", C.c_void_p), ("mate_offset", C.c_void_p), ("mate_length", C.c_void_p),
                ("codes", C.c_void_p), ("codes_length", C.c_int64), ("expected_inner", C.c_void_p), ("deviation", C.c_void_p)]


class XmResult(C.Structure):
    _fields_ = [("num_queries", C.c_int64), ("num_ints", C.c_int64), ("num_dbls", C.c_int64), ("ints", C.POINTER(C.c_int32)),
                ("dbls", C.POINTER(C.c_double)), ("int_off", C.POINTER(C.c_int64)), ("dbl_off", C.POINTER(C.c_int64)),
                ("counters", C.c_int64 * 16), ("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("kernel_launches", C.c_int32), ("reserved", C.c_int32), ("prof", C.c_int64 * 16), ("extra", C.c_int64 * 8)]


class XmFastqText(C.Structure):
    """xm_fastq_text: a block of whole four-line FASTQ records as read from the file(s)."""
    _fields_ = [("text1", C.c_void_p), ("bytes1", C.c_int64), ("records1", C.c_int64), ("text2", C.c_void_p), ("bytes2", C.c_int64), ("records2", C.c_int64),
                ("expected_inner", C.c_double), ("deviation", C.c_double), ("keep_qualities", C.c_int32), ("split_past_size", C.c_int32)]


class XmFastaText(C.Structure):
    """xm_fasta_text: a block of whole FASTA records ('>' header, any number of body lines) as read from the file(s), with its line counts."""
    _fields_ = [("text1", C.c_void_p), ("bytes1", C.c_int64), ("records1", C.c_int64), ("lines1", C.c_int64), ("text2", C.c_void_p), ("bytes2", C.c_int64), ("records2", C.c_int64),
                ("lines2", C.c_int64), ("expected_inner", C.c_double), ("deviation", C.c_double), ("keep_qualities", C.c_int32), ("split_past_size", C.c_int32)]


class XmFastqBatch(C.Structure):
    """xm_fastq_batch: hostio.XmioBatch's fields (pinned host copies of what the kernels built), then the times of the call's three parts."""
    _fields_ = [("num_queries", C.c_int64), ("mate_count", C.POINTER(C.c_int32)), ("mate_offset", C.POINTER(C.c_int64)), ("mate_length", C.POINTER(C.c_int32)),
                ("codes", C.POINTER(C.c_uint8)), ("codes_length", C.c_int64), ("names", C.c_void_p), ("name_off", C.POINTER(C.c_int64)),
                ("quals", C.c_void_p), ("qual_off", C.POINTER(C.c_int64)), ("has_qual", C.POINTER(C.c_uint8)), ("store", C.c_void_p),
                ("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double)]


class XmSamNames(C.Structure):
    """xm_sam_names: the mates' names as hostio.XmioBatch holds them (name_off has 2 * num_queries + 1 entries)."""
    _fields_ = [("names", C.c_void_p), ("name_off", C.c_void_p)]


class XmSamText(C.Structure):
    """xm_sam_text: the SAM records of a batch in a pinned buffer of the library, and the times of the call's three parts."""
    _fields_ = [("text", C.c_void_p), ("bytes", C.c_int64), ("records", C.c_int64), ("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("store", C.c_void_p)]


class XmTestSamJob(C.Structure):
    """xm_test_sam_job (test-only): a batch with its names, contig names and the four result streams, all on the host."""
    _fields_ = [("num_queries", C.c_int64), ("mate_count", C.c_void_p), ("mate_offset", C.c_void_p), ("mate_length", C.c_void_p), ("codes", C.c_void_p), ("codes_length", C.c_int64),
                ("names", C.c_void_p), ("name_off", C.c_void_p), ("num_contigs", C.c_int32), ("reserved", C.c_int32), ("contig_names", C.POINTER(C.c_char_p)),
                ("ints", C.c_void_p), ("dbls", C.c_void_p), ("int_off", C.c_void_p), ("dbl_off", C.c_void_p)]


class XmTestUnalignedJob(C.Structure):
    """xm_test_unaligned_job (test-only): a batch with its names and qualities and the four result streams, all on the host."""
    _fields_ = [("num_queries", C.c_int64), ("mate_count", C.c_void_p), ("mate_offset", C.c_void_p), ("mate_length", C.c_void_p), ("codes", C.c_void_p), ("codes_length", C.c_int64),
                ("names", C.c_void_p), ("name_off", C.c_void_p), ("quals", C.c_void_p), ("qual_off", C.c_void_p), ("has_qual", C.c_void_p), ("num_contigs", C.c_int32), ("reserved", C.c_int32),
                ("ints", C.c_void_p), ("dbls", C.c_void_p), ("int_off", C.c_void_p), ("dbl_off", C.c_void_p)]


class XmBatchSummary(C.Structure):
    """xm_batch_summary: the statistics of a batch's result streams, the penalties of its alignments and its unaligned queries, in pinned buffers of the library."""
    _fields_ = [("num_queries", C.c_int64), ("num_aligned", C.c_int64), ("num_alignments", C.c_int64), ("total_aligned_length", C.c_int64), ("num_indels", C.c_int64),
                ("num_unaligned", C.c_int64), ("unaligned", C.POINTER(C.c_int64)), ("penalties", C.POINTER(C.c_double)),
                ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("store", C.c_void_p)]


class XmRefsRecord(C.Structure):
    """xm_refs_record: one combination of contigs (ids[:n], ascending contig indices) and the queries of the batch with exactly that set."""
    _fields_ = [("count", C.c_int64), ("n", C.c_int32), ("ids", C.c_int32 * 8), ("reserved", C.c_int32)]


class XmRefsCount(C.Structure):
    """xm_refs_count: the queries of a batch counted per combination of contigs, and the contigs of the queries left to the host, in pinned buffers of the library."""
    _fields_ = [("num_queries", C.c_int64), ("num_aligned", C.c_int64), ("num_combinations", C.c_int64), ("records", C.POINTER(XmRefsRecord)),
                ("num_leftover_queries", C.c_int64), ("leftover_offsets", C.POINTER(C.c_int64)), ("leftover_contigs", C.POINTER(C.c_int32)),
                ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("store", C.c_void_p)]


class XmTestPileupJob(C.Structure):
    """xm_test_pileup_job (test-only): the mates of a batch and events of the pile-up, all on the host."""
    _fields_ = [("num_queries", C.c_int64), ("mate_offset", C.c_void_p), ("mate_length", C.c_void_p), ("codes", C.c_void_p), ("codes_length", C.c_int64),
                ("num_events", C.c_int64), ("events", C.c_void_p), ("query_base", C.c_int64)]


class XmMutationFilter(C.Structure):
    """xm_mutation_filter: MutationDetectionParameters - the total-depth thresholds as doubles, the fractions as floats."""
    _fields_ = [("min_snp_total_depth", C.c_double), ("min_indel_total_start_depth", C.c_double), ("min_indel_continuation_total_depth", C.c_double),
                ("min_snp_depth_fraction", C.c_float), ("min_indel_start_depth_fraction", C.c_float), ("min_indel_continuation_depth_fraction", C.c_float), ("reserved", C.c_int32)]


class XmSnpRow(C.Structure):
    """xm_snp_row: a SNP row of the device pile-up (position 0-based in the contig, letter the index into ACGT, the depths in units)."""
    _fields_ = [("contig", C.c_int32), ("position", C.c_int32), ("letter", C.c_uint8), ("reference_code", C.c_uint8), ("reserved", C.c_uint8 * 6),
                ("support_units", C.c_uint64), ("total_units", C.c_uint64)]


SNP_ROW = np.dtype({"names": ["contig", "position", "letter", "reference_code", "support_units", "total_units"], "formats": [np.int32, np.int32, np.uint8, np.uint8, np.uint64, np.uint64],
                    "offsets": [0, 4, 8, 9, 16, 24], "itemsize": 32})  # XmSnpRow as a numpy record
INDEL_CANDIDATE = np.dtype([("contig", np.int32), ("kind", np.int32), ("pos1", np.int64), ("length", np.int64), ("support_units", np.uint64)])  # xm_indel_candidate
INDEL_VERDICT = np.dtype([("total_units", np.uint64), ("keep", np.int64)])  # xm_indel_verdict


class XmSnpCalls(C.Structure):
    """xm_snp_calls: the SNP rows of a pile-up in a pinned buffer of the library, what crossed to the host and the times of the call's two parts."""
    _fields_ = [("num_rows", C.c_int64), ("rows", C.POINTER(XmSnpRow)), ("positions", C.c_int64), ("bytes_to_host", C.c_int64), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double),
                ("store", C.c_void_p)]


class XmTestMutationsJob(C.Structure):
    """xm_test_mutations_job (test-only): contig lengths, one or two sets of counts, a filter and indel candidates, all on the host."""
    _fields_ = [("num_contigs", C.c_int32), ("num_sets", C.c_int32), ("contig_lengths", C.c_void_p), ("depth", C.c_void_p * 2), ("alt", C.c_void_p * 2), ("middle", C.c_void_p * 2),
                ("filter", C.POINTER(XmMutationFilter)), ("num_candidates", C.c_int64), ("candidates", C.c_void_p), ("verdicts", C.c_void_p), ("read_back", C.c_void_p * 2)]


class XmIndelCall(C.Structure):
    """xm_indel_call: a group of insertion / deletion events as xm_pileup_call_indels returns it."""
    _fields_ = [("contig", C.c_int32), ("kind", C.c_int32), ("pos1", C.c_int64), ("length", C.c_int64), ("keep", C.c_int64), ("support_units", C.c_uint64), ("total_units", C.c_uint64),
                ("letters_at", C.c_int64), ("num_letters", C.c_int64)]


INDEL_CALL = np.dtype([("contig", np.int32), ("kind", np.int32), ("pos1", np.int64), ("length", np.int64), ("keep", np.int64), ("support_units", np.uint64), ("total_units", np.uint64),
                       ("letters_at", np.int64), ("num_letters", np.int64)])  # xm_indel_call as a numpy record


class XmIndelCalls(C.Structure):
    """xm_indel_calls: the kept groups of a pile-up and their letters in pinned buffers of the library, and the figures of the table."""
    _fields_ = [("num_rows", C.c_int64), ("rows", C.POINTER(XmIndelCall)), ("num_letters", C.c_int64), ("letters", C.c_void_p), ("groups", C.c_int64), ("events", C.c_int64),
                ("left_over", C.c_int64), ("table_bytes", C.c_int64), ("bytes_to_host", C.c_int64), ("store", C.c_void_p)]


class XmTestGroupCall(C.Structure):
    """xm_test_group_call (test-only): the events of one call with the offsets of their letters and the letters."""
    _fields_ = [("num_events", C.c_int64), ("events", C.c_void_p), ("text_off", C.c_void_p), ("text", C.c_void_p)]


class XmTestGroupJob(C.Structure):
    """xm_test_group_job (test-only): one or two sets of calls, the knobs of the table, and where the left-over events go."""
    _fields_ = [("fingerprint_bits", C.c_int32), ("initial_capacity", C.c_int32), ("num_calls", C.c_int32 * 2), ("calls", C.POINTER(XmTestGroupCall) * 2), ("left_cap", C.c_int64),
                ("left_text_cap", C.c_int64), ("left_events", C.c_void_p), ("left_call", C.c_void_p), ("left_text_off", C.c_void_p), ("left_text", C.c_void_p), ("num_left", C.c_int64),
                ("grows", C.c_int64 * 3)]


def indel_calls(calls):
    """POINTER(XmIndelCalls) -> (xm_indel_call records, their letters as bytes, the figures), copied: the C result can be freed afterwards."""
    got = calls.contents
    n, nl = int(got.num_rows), int(got.num_letters)
    rows = np.frombuffer((XmIndelCall * n).from_address(C.addressof(got.rows.contents)), dtype=INDEL_CALL).copy() if n else np.zeros(0, INDEL_CALL)
    letters = C.string_at(got.letters, nl) if nl else b""
    return rows, letters, {"groups": int(got.groups), "events": int(got.events), "left_over": int(got.left_over), "table_bytes": int(got.table_bytes), "bytes_to_host": int(got.bytes_to_host)}


ABI_VERSION = 12  # include/xmapper_hip.h, xm_abi_version(): xm_result.extra[] appended; xm_seed_probe_packed (the packed output layout under its own name); 3: xm_context_set_collapse, extra[7]; 4: xm_context_set_memo, xm_context_memo_info, extra[6]; 5: xm_memory_new, xm_context_attach_memory, xm_memory_info, xm_memory_free; 6: xm_batch_stage_fastq, xm_fastq_batch_free, xm_fastq_tile_bytes; 7: xm_sam_set_contigs, xm_sam_format_last, xm_sam_text_free, xm_sam_tile_bytes, xm_test_sam_format, xm_test_format_doubles; 8: xm_batch_unstage; 9: xm_pileup_keep_insert_text, xm_pileup_event_text, xm_test_pileup_text; 10: xm_context_set_result_copy, xm_summary_last, xm_summary_free, xm_test_summary; 11: xm_refs_count_last, xm_refs_count_free, xm_test_refs_count; 12: xm_fastq_text.split_past_size (was reserved); xm_batch_stage_fasta came without a new version (no struct or entry changed), and so did xm_unaligned_format_last, xm_context_set_batch_copy and xm_test_unaligned_format, and xm_pileup_absorb, xm_pileup_call_snps, xm_snp_calls_free, xm_pileup_judge_indels, xm_mutations_block_positions and xm_test_pileup_call, and xm_pileup_group_events, xm_pileup_call_indels, xm_indel_calls_free and xm_test_pileup_group


class XmIndexInfo(C.Structure):
    _fields_ = [("num_contigs", C.c_int32), ("min_interesting_size", C.c_int32), ("max_hashed_length", C.c_int32), ("enable_gapmers", C.c_int32),
                ("dup_window", C.c_int32), ("position_bytes", C.c_int32), ("total_forward_size", C.c_int64), ("index_bytes", C.c_int64),
                ("num_positions", C.c_int64), ("dup_granularity", C.c_double), ("built_on_device", C.c_int32), ("bucket_line_bytes", C.c_int32),
                ("hash_seconds", C.c_double), ("duplication_seconds", C.c_double)]


EXPORTS = ["xm_last_error", "xm_build_stamp", "xm_abi_version", "xm_pinned_host_bytes", "xm_device_count", "xm_index_build", "xm_index_replicate", "xm_context_new", "xm_context_set_scratch", "xm_context_set_collapse", "xm_context_set_memo", "xm_context_memo_info", "xm_memory_new", "xm_context_attach_memory", "xm_memory_info", "xm_memory_free", "xm_device_memory", "xm_index_save", "xm_index_load", "xm_index_ensure_length", "xm_index_free", "xm_index_get_info",
           "xm_index_table_info", "xm_index_table_shape", "xm_index_table_dump", "xm_index_bucket_stats", "xm_index_dup_keys", "xm_align_batch", "xm_result_free", "xm_batch_upload", "xm_batch_stage", "xm_batch_commit", "xm_batch_unstage", "xm_batch_stage_fastq", "xm_batch_stage_fasta", "xm_fastq_batch_free", "xm_fastq_tile_bytes", "xm_sam_set_contigs", "xm_sam_format_last", "xm_sam_text_free", "xm_sam_tile_bytes", "xm_test_sam_format", "xm_test_format_doubles", "xm_align_resident", "xm_seed_probe_packed", "xm_measure_random_gather", "xm_test_local_align", "xm_test_bound_counters", "xm_test_bound", "xm_pileup_new", "xm_pileup_set_query_ends", "xm_pileup_read_middle", "xm_pileup_add_last", "xm_pileup_read", "xm_pileup_events", "xm_pileup_keep_insert_text", "xm_pileup_event_text", "xm_test_pileup_text", "xm_pileup_free", "xm_context_set_result_copy", "xm_summary_last", "xm_summary_free", "xm_test_summary", "xm_refs_count_last", "xm_refs_count_free", "xm_test_refs_count", "xm_unaligned_format_last", "xm_context_set_batch_copy", "xm_test_unaligned_format",
           "xm_pileup_absorb", "xm_pileup_call_snps", "xm_snp_calls_free", "xm_pileup_judge_indels", "xm_mutations_block_positions", "xm_test_pileup_call",
           "xm_pileup_group_events", "xm_pileup_call_indels", "xm_indel_calls_free", "xm_test_pileup_group", "xm_test_scan"]


def build_library(force=False):
    """Compile libxmapper_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "xmapper_hip.h")]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-j8", "-C", CSRC], stdout=subprocess.DEVNULL)
    return LIB_PATH


def source_stamp():
    """The digest the Makefile compiles into the library (xm_build_stamp): SHA-256 over csrc/*.h, *.hip in name order, then include/xmapper_hip.h."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(f for f in os.listdir(CSRC) if f.endswith(".h") or f.endswith(".hip")):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(os.path.join(HERE, "..", "include", "xmapper_hip.h"), "rb").read())
    return h.hexdigest()[:16]


def build_stamp():
    return lib().xm_build_stamp().decode()


def check_stamp():
    """Raises when the loaded library was not built from the sources in this tree."""
    have, want = build_stamp(), source_stamp()
    if have != want:
        raise RuntimeError("libxmapper_hip.so is stale: built from sources %s, the tree holds %s (run make -j8 -C mapper_amd/csrc)" % (have, want))
    return have


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("XM_LIB_PATH") or LIB_PATH  # (XM_LIB_PATH: A/B experiments with another build of the same library)
        if not os.path.exists(path):
            # no lazy build here: a process that runs under a profiler's preloaded library must not start make/hipcc children
            # (and a half-built library must never be picked up silently); __graft_entry__.build() or `make -C mapper_amd/csrc` builds it
            raise ImportError("%s is missing: build it first (python -c 'import __graft_entry__ as g; g.build()' or make -j8 -C mapper_amd/csrc); "
                              "mapper_amd has no CPU fallback" % path)
        L = C.CDLL(path)  # (XM_LIB_PATH: A/B experiments with another build of the same library)
        if not hasattr(L, "xm_abi_version") or L.xm_abi_version() != ABI_VERSION:
            raise ImportError("%s implements another version of include/xmapper_hip.h than this binding (%d): rebuild it (make -j8 -C mapper_amd/csrc)" % (path, ABI_VERSION))
        L.xm_last_error.restype = C.c_char_p
        L.xm_build_stamp.restype = C.c_char_p
        L.xm_pinned_host_bytes.restype = C.c_int64
        L.xm_pinned_host_bytes.argtypes = [C.POINTER(C.c_int64)]
        L.xm_index_build.argtypes = [C.POINTER(XmRef), C.POINTER(XmBuildOpts), C.POINTER(C.c_void_p)]
        L.xm_index_save.argtypes = [C.c_void_p, C.c_char_p]
        L.xm_index_replicate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.xm_context_new.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.xm_context_set_scratch.argtypes = [C.c_void_p, C.c_int64]
        L.xm_context_set_collapse.argtypes = [C.c_void_p, C.c_int32]
        L.xm_context_set_memo.argtypes = [C.c_void_p, C.c_int64]
        L.xm_context_memo_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_memory_new.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        L.xm_context_attach_memory.argtypes = [C.c_void_p, C.c_void_p]
        L.xm_memory_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_memory_free.argtypes = [C.c_void_p]
        L.xm_memory_free.restype = None
        L.xm_device_memory.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_index_load.argtypes = [C.c_char_p, C.POINTER(XmRef), C.POINTER(XmBuildOpts), C.POINTER(C.c_void_p)]
        L.xm_index_ensure_length.argtypes = [C.c_void_p, C.c_int32]
        L.xm_index_free.argtypes = [C.c_void_p]
        L.xm_index_get_info.argtypes = [C.c_void_p, C.POINTER(XmIndexInfo)]
        L.xm_index_table_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_index_table_shape.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.xm_index_bucket_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.xm_index_table_dump.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.xm_index_dup_keys.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.xm_index_dup_keys.restype = C.c_int64
        L.xm_align_batch.argtypes = [C.c_void_p, C.POINTER(XmParams), C.POINTER(XmQueryBatch), C.POINTER(C.POINTER(XmResult))]
        L.xm_result_free.argtypes = [C.POINTER(XmResult)]
        L.xm_batch_upload.argtypes = [C.c_void_p, C.POINTER(XmQueryBatch)]
        L.xm_batch_stage.argtypes = [C.c_void_p, C.POINTER(XmQueryBatch)]
        L.xm_batch_commit.argtypes = [C.c_void_p]
        L.xm_batch_unstage.argtypes = [C.c_void_p]
        L.xm_batch_stage_fastq.argtypes = [C.c_void_p, C.POINTER(XmFastqText), C.POINTER(C.POINTER(XmFastqBatch))]
        L.xm_batch_stage_fasta.argtypes = [C.c_void_p, C.POINTER(XmFastaText), C.POINTER(C.POINTER(XmFastqBatch))]  # (added without a new ABI version: include/xmapper_hip.h)
        L.xm_fastq_batch_free.argtypes = [C.POINTER(XmFastqBatch)]
        L.xm_fastq_batch_free.restype = None
        L.xm_sam_set_contigs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
        L.xm_sam_format_last.argtypes = [C.c_void_p, C.POINTER(XmSamNames), C.POINTER(C.POINTER(XmSamText))]
        L.xm_sam_text_free.argtypes = [C.POINTER(XmSamText)]
        L.xm_sam_text_free.restype = None
        L.xm_test_sam_format.argtypes = [C.c_int32, C.POINTER(XmTestSamJob), C.POINTER(C.POINTER(XmSamText))]
        L.xm_test_format_doubles.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xm_align_resident.argtypes = [C.c_void_p, C.POINTER(XmParams), C.POINTER(C.POINTER(XmResult))]
        L.xm_seed_probe_packed.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.xm_measure_random_gather.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_double)]
        L.xm_test_local_align.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(XmParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                          C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_test_bound_counters.argtypes = [C.POINTER(C.c_int64)]
        L.xm_test_bound_counters.restype = None
        L.xm_test_bound.argtypes = [C.c_int32, C.POINTER(XmParams), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(C.c_int64)]
        L.xm_pileup_new.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.xm_pileup_set_query_ends.argtypes = [C.c_void_p, C.c_double]
        L.xm_pileup_read_middle.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
        L.xm_pileup_add_last.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.xm_pileup_read.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.xm_pileup_events.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.xm_pileup_events.restype = C.c_int64
        L.xm_pileup_keep_insert_text.argtypes = [C.c_void_p, C.c_int32]
        L.xm_pileup_event_text.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
        L.xm_pileup_event_text.restype = C.c_int64
        L.xm_test_pileup_text.argtypes = [C.c_int32, C.POINTER(XmTestPileupJob), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.xm_pileup_free.argtypes = [C.c_void_p]
        L.xm_context_set_result_copy.argtypes = [C.c_void_p, C.c_int32]
        L.xm_summary_last.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(XmBatchSummary))]
        L.xm_summary_free.argtypes = [C.POINTER(XmBatchSummary)]
        L.xm_summary_free.restype = None
        L.xm_test_summary.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(XmBatchSummary))]
        L.xm_refs_count_last.argtypes = [C.c_void_p, C.POINTER(C.POINTER(XmRefsCount))]
        L.xm_refs_count_free.argtypes = [C.POINTER(XmRefsCount)]
        L.xm_refs_count_free.restype = None
        L.xm_test_refs_count.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(XmRefsCount))]
        L.xm_unaligned_format_last.argtypes = [C.c_void_p, C.POINTER(C.POINTER(XmSamText))]  # (added without a new ABI version, as xm_batch_stage_fasta)
        L.xm_context_set_batch_copy.argtypes = [C.c_void_p, C.c_int32]
        L.xm_test_unaligned_format.argtypes = [C.c_int32, C.POINTER(XmTestUnalignedJob), C.POINTER(C.POINTER(XmSamText))]
        L.xm_pileup_absorb.argtypes = [C.c_void_p, C.c_void_p]  # (these six, too, came without a new ABI version)
        L.xm_pileup_call_snps.argtypes = [C.c_void_p, C.POINTER(XmMutationFilter), C.POINTER(C.POINTER(XmSnpCalls))]
        L.xm_snp_calls_free.argtypes = [C.POINTER(XmSnpCalls)]
        L.xm_snp_calls_free.restype = None
        L.xm_pileup_judge_indels.argtypes = [C.c_void_p, C.POINTER(XmMutationFilter), C.c_void_p, C.c_int64, C.c_void_p]
        L.xm_mutations_block_positions.restype = C.c_int64
        L.xm_test_pileup_call.argtypes = [C.c_int32, C.POINTER(XmTestMutationsJob), C.POINTER(C.POINTER(XmSnpCalls))]
        L.xm_pileup_group_events.argtypes = [C.c_void_p, C.c_int32]  # (these four, too, came without a new ABI version)
        L.xm_pileup_call_indels.argtypes = [C.c_void_p, C.POINTER(XmMutationFilter), C.POINTER(C.POINTER(XmIndelCalls))]
        L.xm_indel_calls_free.argtypes = [C.POINTER(XmIndelCalls)]
        L.xm_indel_calls_free.restype = None
        L.xm_test_pileup_group.argtypes = [C.c_int32, C.POINTER(XmTestGroupJob), C.POINTER(C.POINTER(XmIndelCalls))]
        L.xm_test_scan.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]  # (test-only: no new ABI version)
        _lib = L
    return _lib


def make_ref(contigs):
    """contigs: list of (name, uint8 code array).  Returns (XmRef, keepalive)."""
    n = len(contigs)
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in contigs])
    arrays = [np.ascontiguousarray(c, dtype=np.uint8) for _, c in contigs]
    codes = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
    lengths = (C.c_int64 * n)(*[len(a) for a in arrays])
    ref = XmRef(n, names, codes, lengths)
    return ref, (names, arrays, codes, lengths)


def make_batch(mate_count, mate_offset, mate_length, codes, expected_inner, deviation):
    arrs = (np.ascontiguousarray(mate_count, dtype=np.int32), np.ascontiguousarray(mate_offset, dtype=np.int64),
            np.ascontiguousarray(mate_length, dtype=np.int32), np.ascontiguousarray(codes, dtype=np.uint8),
            np.ascontiguousarray(expected_inner, dtype=np.float64), np.ascontiguousarray(deviation, dtype=np.float64))
    b = XmQueryBatch(len(arrs[0]), arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, len(arrs[3]),
                     arrs[4].ctypes.data, arrs[5].ctypes.data)
    return b, arrs


def copy_result(r):
    """XmResult -> dict of numpy arrays (copies; the C result can be freed afterwards)."""
    ints = np.ctypeslib.as_array(r.ints, shape=(max(r.num_ints, 1),))[:r.num_ints].copy()
    dbls = np.ctypeslib.as_array(r.dbls, shape=(max(r.num_dbls, 1),))[:r.num_dbls].copy()
    io = np.ctypeslib.as_array(r.int_off, shape=(r.num_queries + 1,)).copy()
    do = np.ctypeslib.as_array(r.dbl_off, shape=(r.num_queries + 1,)).copy()
    return dict(ints=ints, dbls=dbls, int_off=io, dbl_off=do, counters=list(r.counters), kernel_ms=r.kernel_ms, h2d_ms=r.h2d_ms,
                d2h_ms=r.d2h_ms, kernel_launches=r.kernel_launches, prof=list(r.prof), extra=list(r.extra),
                memory_wait_us=int(r.reserved))  # (xm_result.reserved: host microseconds the call waited for its memory's mutex)


class _ResultOwner:
    """Frees the C result when the last numpy view of its streams is gone."""

    def __init__(self, L, res):
        self._L, self._res = L, res

    def __del__(self):
        try:
            self._L.xm_result_free(self._res)
        except Exception:
            pass


def view_result(L, res):
    """POINTER(XmResult) -> dict of numpy arrays that alias the (pinned) C streams: no copy of the ~100 MB a 1M-read batch
    returns.  Every array keeps the owner alive through its ctypes base object; the owner frees the result."""
    r = res.contents
    owner = _ResultOwner(L, res)

    def view(ptr, ctype, n):
        if not ptr:  # (xm_context_set_result_copy(0): the streams stayed in HBM; with no view to hold it the owner frees the result when this returns)
            return None
        buf = (ctype * max(int(n), 1)).from_address(C.addressof(ptr.contents))
        buf._xm_owner = owner
        return np.frombuffer(buf, dtype=np.dtype(ctype))[:int(n)]

    return dict(ints=view(r.ints, C.c_int32, r.num_ints), dbls=view(r.dbls, C.c_double, r.num_dbls), int_off=view(r.int_off, C.c_int64, r.num_queries + 1),
                dbl_off=view(r.dbl_off, C.c_int64, r.num_queries + 1), counters=list(r.counters), kernel_ms=r.kernel_ms, h2d_ms=r.h2d_ms,
                d2h_ms=r.d2h_ms, kernel_launches=r.kernel_launches, prof=list(r.prof), extra=list(r.extra),
                memory_wait_us=int(r.reserved),  # (xm_result.reserved: host microseconds the call waited for its memory's mutex)
                num_queries=int(r.num_queries), num_ints=int(r.num_ints), num_dbls=int(r.num_dbls))


def pinned_host_bytes():
    """(bytes of page-locked host memory the library's result-buffer pool holds now, the most it ever held) in this process."""
    hw = C.c_int64()
    now = lib().xm_pinned_host_bytes(C.byref(hw))
    return int(now), int(hw.value)
