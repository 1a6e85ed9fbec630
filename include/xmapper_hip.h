/* xmapper_hip.h — C ABI of libxmapper_hip.so: the MI355X-native drop-in for X-Mapper's per-read seed-and-extend path.
 *
 * The reference (mathjeff/Mapper, 100 % Java) has no FFI seam; the narrowest stable boundary on this path is
 *     AlignerWorker.align(Query) -> QueryAlignments          src/main/java/mapper/AlignerWorker.java:256-261
 *     (batch form: the loop of AlignerWorker.process()        src/main/java/mapper/AlignerWorker.java:177-231)
 * which is also the public Api.align(Query, ReferenceDatabase, AlignmentParameters, Logger)   Api.java:79-92.
 * Every entry point below cites the reference code it replaces.  INTEGRATION.md shows the JNI binding a maintainer
 * would add on the Java side.  Plain pointers and sizes only; no Java, torch or C++ types cross this boundary.
 *
 * Bases are 4-bit IUPAC masks, one per byte: A=1 C=2 G=4 T=8, ambiguity = OR (QuickVariants Basepairs encoding, see
 * HashBlock_Matcher.java:184-196).  Contigs are passed forward-only in the order Mapper.sortAndComplementReference
 * produces (Mapper.java:1151-1172: length-descending); the reverse complements are implied.
 *
 * Errors: like the reference (any worker exception aborts the run, AlignerWorker.java:195-197, Mapper.java:1070-1077)
 * a failing call returns non-zero, produces no partial result, and xm_last_error() describes it.
 * Threading: the reference shares one HashBlock_Database between all AlignerWorker threads through per-thread views
 * (HashBlock_Database.java:129-133, Mapper.java:1026-1040; Api.java:78 "thread-safe").  Here an xm_index handle is one such view - a CONTEXT:
 * its own HIP stream, batch buffers, scratch and result pool over tables that every context of the index shares (host tables: all contexts;
 * tables in HBM: the contexts of one GPU).  Calls on one context serialise; contexts run side by side, one host thread each
 * (xm_context_new for a further context on the same GPU, xm_index_replicate for one on another GPU).  Tables that grow
 * (xm_index_ensure_length, a batch with longer mates) grow for every context; the launches that read them are waited for.
 */
#ifndef XMAPPER_HIP_H
#define XMAPPER_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* AlignmentParameters (AlignmentParameters.java:8-35).  StartingInsertionStartFree is always false at entry. */
typedef struct xm_params {
  double MutationPenalty, InsertionStart_Penalty, InsertionExtension_Penalty, DeletionStart_Penalty, DeletionExtension_Penalty,
      MaxErrorRate, UnalignedPenalty, AmbiguityPenalty, Max_PenaltySpan;
  int32_t MaxNumMatches;
  int32_t reserved;
} xm_params;

typedef struct xm_ref {
  int32_t num_contigs;
  const char* const* names;      /* may be NULL */
  const uint8_t* const* codes;   /* [num_contigs] forward strand */
  const int64_t* lengths;        /* [num_contigs] */
} xm_ref;

/* How the reference database is assembled (Mapper.java:657-692 vs Api.java:41-69). */
typedef struct xm_build_opts {
  int32_t enable_gapmers;        /* 1 (default); 0 = --no-gapmers (Mapper.java:245) */
  int32_t min_interesting_size;  /* <=0: (int)max(log4(N+1)-2, 1)  (HashBlock_Database.java:52) */
  int32_t max_hashed_length;     /* <=0: chooseMaxDuplicationLength = 2*ceil(log2 N) (DuplicationDetector.java:17-36); grows on demand */
  int32_t dup_window;            /* 1000 for Mapper.run (Mapper.java:691), 1 for Api.newDatabase (Api.java:66) */
  int32_t dup_min_copies;        /* 2 */
  int32_t dup_min_length;        /* <=0: chooseMinDuplicationLength */
  int32_t dup_max_length;        /* <=0: chooseMaxDuplicationLength */
  int32_t device;                /* HIP device ordinal; <0: current device */
  int32_t host_only;             /* 1: build the host-side tables only (no GPU touched): index inspection on CPU-only machines */
  int32_t reserved;
} xm_build_opts;

typedef struct xm_index xm_index;

/* A batch of queries = the List<QueryBuilder> one AlignerWorker.process() call consumes (AlignerWorker.java:177). */
typedef struct xm_query_batch {
  int64_t num_queries;
  const int32_t* mate_count;     /* [nq] 1 or 2 (Query.getNumSequences()) */
  const int64_t* mate_offset;    /* [2*nq] offset of each mate in `codes` */
  const int32_t* mate_length;    /* [2*nq] */
  const uint8_t* codes;          /* mates as given in the FASTQ (mate 2 NOT reverse-complemented) */
  int64_t codes_length;
  const double* expected_inner;  /* [nq] Query.getExpectedInnerDistance() (paired only; --spacing, Mapper.java:34) */
  const double* deviation;       /* [nq] Query.getSpacingDeviationPerUnitPenalty() (Mapper.java:35) */
} xm_query_batch;

/* Results = List<QueryAlignments> (AlignerWorker.java:231,652-656) flattened into two streams.
 * For query q, ints[int_off[q] .. int_off[q+1]) and dbls[dbl_off[q] .. dbl_off[q+1]) hold, in this order:
 *   ints: numComponents (1; 2 when a pair fell back to unpaired alignments, AlignerWorker.java:643)
 *         per component: numAlignments
 *           per alignment (= QueryAlignment ctor args, QueryMatch_Aligner.java:267): innerDistance, numSequences
 *             per sequence (= SequenceAlignment): contigIndex, referenceReversed, numBlocks,
 *               per block (= AlignedBlock): startA, startB, lengthA, lengthB
 *   dbls:   per alignment: spacingPenalty, overlapMultiplier, duplicationBonus, totalPenalty
 *             per sequence: totalPenalty, alignedPenalty
 * An unaligned query is one component with zero alignments (QueryAlignments.unaligned, AlignerWorker.java:480). */
typedef struct xm_result {
  int64_t num_queries, num_ints, num_dbls;
  int32_t* ints;
  double* dbls;
  int64_t* int_off;  /* [nq+1] */
  int64_t* dbl_off;  /* [nq+1] */
  /* counters of this call: 0 reads, 1 bucket-header probes (PackedMap.getNumMatchesLowerBound), 2 bucket fetches (PackedMap.get),
   * 3 positions fetched, 4 candidates extended (QueryMatch_Aligner.doAlign), 5 PathAligner calls, 6 PathAligner nodes, 7 quick accepts,
   * 8 alignments written, 9 reference-window bytes (4-bit), 10 read bytes (4-bit), 11 reads rerun with a larger scratch scale,
   * 12-15 kernel microseconds by pass: 12 wave-per-read light tier (+ lane-per-read light pass of what the wave form left), 13 wave-per-read
   * chain tier, 14 wave-per-read search tier, 15 lane-per-read gapped / rerun passes */
  int64_t counters[16];
  double kernel_ms;   /* sum of the align (and search, collapse and memory) kernels' launch durations (HIP events on the launch stream) */
  double h2d_ms, d2h_ms;  /* batch upload; prefix sums + query-order gather + copy of the four streams to the host */
  int32_t kernel_launches;  /* align + search (+ collapse, + memory) kernel launches of this call */
  int32_t reserved;  /* (ABI version 5) microseconds of host time this call waited for the mutex of its memory of aligned queries (both critical sections; 0 without one) */
  int64_t prof[16];   /* diagnostic builds (-DXM_PROFILE=1: summed over lanes, =2: per wave) only: shader-clock ticks per phase; otherwise 0 */
  /* (appended in ABI version 2; xm_abi_version())  the rejection filter in front of PathAligner (batches of long reads): 0 searches it examined, 1 searches it
   * proved null without running them (PathAligner.java:169: the search would have returned null after exploring every node within the budget; their nodes
   * are not in counters[6]), 2 cells of the bounding recurrence it computed, 3 = 1 when a pass of this call ran with the filter; 4 pieces (BlockAligner.alignPiece,
   * BlockAligner.java:215-249) the filter examined, 5 pieces it proved unalignable within their budget before their chain ran (their PathAligner calls and nodes are in neither counters[5] nor
   * counters[6]); 6 (ABI version 4) queries of this call whose results were replayed from the context's memory of
   * earlier calls - or, with xm_context_attach_memory, from the GPU's memory, either generation - instead of being aligned (xm_context_set_memo; 0 when it is off); 7 (ABI version 3) queries of this call whose results were copied from a byte-identical query of the batch instead of being
   * aligned (xm_context_set_collapse; 0 when collapsing is off) */
  int64_t extra[8];
} xm_result;

typedef struct xm_index_info_t {
  int32_t num_contigs, min_interesting_size, max_hashed_length, enable_gapmers, dup_window, position_bytes;
  int64_t total_forward_size, index_bytes, num_positions;
  double dup_granularity;
  int32_t built_on_device;       /* 1: the tables were hashed on the GPU (xm_index_device.hip), 0: by the host builder (or read from a file) */
  int32_t bucket_line_bytes;     /* 32 / 64: the index has bucket lines of that size in HBM (a probe is one access: xm_seed_probe_lines_kernel); 0: CSR arrays only (xm_seed_probe_kernel) */
  double hash_seconds;           /* wall time of hashing the reference into tables (all calls so far), */
  double duplication_seconds;    /* and of the duplication map */
} xm_index_info_t;

const char* xm_last_error(void);
/* First 16 hex digits of the SHA-256 over the library's sources (every .h and .hip file of mapper_amd/csrc in name order, then this header) at build
 * time: lets a caller check that the loaded library was built from the sources it sits beside. */
const char* xm_build_stamp(void);
/* Version of this header's structs and entry points: 2 = xm_result.extra[] appended, xm_seed_probe_packed replaces xm_seed_probe; 3 = xm_context_set_collapse,
 * xm_result.extra[7]; 4 = xm_context_set_memo, xm_context_memo_info, xm_result.extra[6]; 5 = xm_memory_new, xm_context_attach_memory, xm_memory_info,
 * xm_memory_free, xm_result.reserved carries the wait for a memory; 6 = xm_batch_stage_fastq, xm_fastq_batch_free, xm_fastq_tile_bytes; 7 = xm_sam_set_contigs,
 * xm_sam_format_last, xm_sam_text_free, xm_sam_tile_bytes (and the test-only xm_test_sam_format, xm_test_format_doubles); 8 = xm_batch_unstage; 9 = xm_pileup_keep_insert_text, xm_pileup_event_text (and the test-only
 * xm_test_pileup_text); 10 = xm_context_set_result_copy, xm_summary_last, xm_summary_free (and the test-only xm_test_summary);
 * 11 = xm_refs_count_last, xm_refs_count_free (and the test-only xm_test_refs_count); 12 = xm_fastq_text.reserved becomes split_past_size (same layout; 0 is
 * what every caller passed).  xm_batch_stage_fasta was added without a new version: it changes no struct and no entry, so the version stays 12 and a
 * caller that wants it looks the symbol up (a library of version 12 built before it does not export it); xm_pileup_absorb, xm_pileup_call_snps,
 * xm_snp_calls_free, xm_pileup_judge_indels and xm_mutations_block_positions (and the test-only xm_test_pileup_call) came the same way, and so did
 * xm_pileup_group_events, xm_pileup_call_indels and xm_indel_calls_free (and the test-only xm_test_pileup_group).  A binding checks the version once
 * after loading the library (mapper_amd/_capi.py, bindings/java/xmapper_jni.c). */
int32_t xm_abi_version(void);
/* Page-locked host memory this process holds through the library's pool of result buffers (in use + kept for reuse; at most 4 GiB are kept idle), and - through
 * high_water, if not NULL - the most it ever held.  Eight ranks of a node, each with several contexts, all pin host memory: bench.py prints the mark per rank. */
int64_t xm_pinned_host_bytes(int64_t* high_water);
int xm_device_count(void);

/* Replaces new SequenceDatabase + new HashBlock_Database(...).prepare() + new DuplicationDetector(...).helpSetup()
 * (Mapper.java:657-692, Api.java:41-69, HashBlock_Database.java:490-665, PackedMap.java:54-153, DuplicationDetector.java:97-436)
 * and uploads the result to HBM. */
int xm_index_build(const xm_ref* ref, const xm_build_opts* opts, xm_index** out);
/* A further context of a built index (see "Threading" above).  xm_context_new: on the source's GPU; host tables and tables in HBM are the
 * source's own (no copy of either: a 3 Gb reference's ~130 GB of tables and bucket lines exist once per GPU however many contexts align on it).
 * xm_index_replicate: on `device`; the host tables are shared, and when `device` is another GPU the tables are copied from the source's HBM
 * (hipMemcpyPeer: xGMI between GPUs) instead of being built or uploaded again (device == the source's: the same as xm_context_new).  The
 * reference shares one HashBlock_Database between all AlignerWorkers of a run (Mapper.java:912-1134); one copy per GPU is that sharing here
 * (index replicated, reads sharded, no collective).  Every handle is released with xm_index_free, in any order: the
 * shared tables go with the last one. */
int xm_context_new(xm_index* source, xm_index** out);
int xm_index_replicate(xm_index* source, int32_t device, xm_index** out);
/* Upper limit of the scratch (HBM) a context may allocate for its passes (0: the default, up to 200 GiB).  A context never takes more than 3/4
 * of what is free when it sizes its scratch, and settles for less when the allocation fails; callers that run several contexts on one GPU divide
 * what xm_device_memory reports as free (after the index is resident) between them.  No reference counterpart (the JVM's -Xmx is the analogue). */
int xm_context_set_scratch(xm_index* context, int64_t bytes);
int xm_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);
/* Identical queries of a batch aligned once (AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291: the reference looks every query up in its
 * run-wide AlignmentCache and binds the cached alignments to the new query).  Per context, off by default.  With enable != 0 every align call of this
 * context (xm_align_batch, xm_align_resident after xm_batch_upload or xm_batch_commit) aligns one query of each group of byte-identical queries of the batch
 * - same mate count, same mate lengths and bytes in order, same bit patterns of expected_inner and deviation - namely the one with the lowest index, and
 * gives every other query of the group a copy of its results: the streams are the same as with collapsing off.  Queries that are identical only across
 * batches are aligned in each.  What changes is the meaning of the work counters: counters[0..10] and extra[0..5] then count the work done, for the
 * aligned queries only, and extra[7] the queries served as copies.  That is why it is not on by default: bench.py and the GPU tests compare those
 * counters with the oracle read by read.  "Failed to align query q" names the lowest index of the group. */
int xm_context_set_collapse(xm_index* context, int32_t enable);
/* The run-wide half of the same cache (AlignmentCache.java spans the run, not a batch).  max_bytes > 0 gives this context a memory of that many bytes of HBM
 * (a fingerprint table and an arena of records; at least 65 536 bytes, less fails); 0 switches it off and frees it; setting it again forgets what it held.
 * With it, every later align call of the context looks each query up first and serves it from a byte-identical query - identical as above - that THIS
 * context aligned in an earlier call under bit-identical xm_params; whatever it aligns itself it remembers afterwards, until the memory is full (nothing
 * is evicted: full means nothing more is remembered).  The memory implies the within-batch collapse for the context.  The four streams are the same as
 * without it.  A call whose xm_params differ in any bit from the ones the memory was filled under empties it first; a call that fails remembers nothing;
 * the memory survives xm_index_ensure_length and growth of the tables by another context (a read only reads the tables of lengths up to its own).
 * Counters: extra[6] = the queries served from the memory, extra[7] = the within-batch copies, counters[0] = num_queries - extra[6] - extra[7], and
 * counters[0..10], extra[0..5] count the work done, as with collapsing.  Per context: a query seen k times over N contexts is aligned at most min(k, N)
 * times (one memory for all contexts of a GPU, which also keeps remembering when it is full: xm_memory_new below).  Off by default.  A non-zero size
 * fails on a context that is attached to a shared memory. */
int xm_context_set_memo(xm_index* context, int64_t max_bytes);
/* out[0] queries remembered, out[1] bytes of HBM in use for them (the table and the records), out[2] the most queries the table takes (the records' arena
 * may fill first), out[3] how often a change of xm_params emptied the memory.  All 0 while the memory is off (out[3] keeps counting over the context's life). */
int xm_context_memo_info(xm_index* context, int64_t out[4]);
/* One memory of aligned queries per GPU, shared and never full (the reference's AlignmentCache is one map for the whole run that every AlignerWorker reads and
 * fills, Api.java:62,82, AlignerWorker.java:264-291).  xm_memory_new makes a memory of max_bytes of HBM on the GPU of `context`, for the contexts of that index
 * on that GPU; it belongs to no context.  generations = 1 or 2: every generation is a table and an arena as above for max_bytes / generations (at least
 * generations * 65 536 bytes, less fails).  xm_context_attach_memory: this context looks its queries up in `memory` and remembers what it aligns there, as
 * with xm_context_set_memo (the within-batch collapse included); NULL detaches.  It fails - xm_last_error says which case - for a context of another index
 * or another GPU (the records depend on the tables), for a context that has xm_context_set_memo on, and for host_only.
 * The rules (mapper_amd/csrc/xm_memo_plan.h states them as code):
 *   lookup   the young generation is probed first, then the old one; a key match whose record is another query does not end the lookup; a query held in
 *            both is served from the young one.
 *   insert   before it, the call knows the exact number of queries it aligned and the exact bytes of their records.  If the young generation takes all of
 *            them they are inserted; otherwise, with two generations and a young one that is not empty, the generations TURN first - the old one is dropped,
 *            the young becomes the old, the dropped one is emptied and becomes the young.  A batch larger than a generation is inserted as far as room goes.
 *            With one generation nothing ever turns: full means nothing more is remembered.
 *   second   the queries a call was served from the old generation only are copied into the young one, if it takes all of them (else none in that call;
 *   chance   never a turn): queries that keep coming back survive the turns.
 *   params   one set per memory: a call from any attached context whose xm_params differ in any bit empties both generations first.
 * The one concurrency rule: launches of different contexts never touch a memory at the same time.  The memory carries a host mutex, which a call holds
 * twice: from before its lookup until replay and promotion have completed on its stream, and from before it measures what it aligned until the insert (and a
 * turn's clears) have completed on its stream.  Between the two, while the passes run, the mutex is free, so the contexts of a GPU keep overlapping their
 * passes; another context may meanwhile insert the same query (the later insert is dropped) or turn the generations.  Results never change: a query is only
 * ever served from a byte-identical query aligned earlier under bit-identical parameters.
 * Lifetime: the memory lives until its handle is freed AND its last context has detached or been freed, in any order; all of its HBM is back with the GPU
 * after that.  xm_memory_info: out[0] records held, 1 bytes of HBM in use (tables and records), 2 records the tables take, 3 times a change of xm_params
 * emptied it, 4 turns of the generations, 5 records promoted, 6 contexts attached, 7 generations. */
typedef struct xm_memory xm_memory;
int xm_memory_new(xm_index* context, int64_t max_bytes, int32_t generations, xm_memory** out);
int xm_context_attach_memory(xm_index* context, xm_memory* memory);
int xm_memory_info(xm_memory* memory, int64_t out[8]);
void xm_memory_free(xm_memory* memory);
/* Binary index cache, in the spirit of --cache-dir (DirCache.java:19-60, HashBlock_Database.java:106-114,477-487, PackedMap.java:249-279:
 * the reference writes one "length-<n>" file per PackedMap under a directory keyed by its property map).  xm_index_save writes the
 * reference, every table hashed so far and the duplication map into ONE file (beside `path`, then renamed: concurrent writers are safe).
 * xm_index_load reads it back and uploads it; with `ref` non-null the file must hold exactly that reference and have been built with the
 * settings `opts` asks for (the reference's cache keys: enableGapmers, minInterestingSize, maxNumShortMatches, format version; plus the
 * duplication settings), else the call fails and the caller builds.  opts->max_hashed_length beyond the file's grows the tables. */
int xm_index_save(xm_index* index, const char* path);
int xm_index_load(const char* path, const xm_ref* ref, const xm_build_opts* opts, xm_index** out);
/* Readable_HashBlock_Database.getContainingMap's lazy growth (Readable_HashBlock_Database.java:108-113): hash tables
 * through gapmers that use `length` bases.  xm_align_batch calls this itself for the longest mate of the batch. */
int xm_index_ensure_length(xm_index* index, int32_t length);
void xm_index_free(xm_index* index);
int xm_index_get_info(const xm_index* index, xm_index_info_t* info);
/* Diagnostics: buckets of all hashed tables, buckets that hold at least one position, buckets marked overfull (more than max(L^2, 5) entries: their positions
 * are dropped, HashBlock_Database.java:569-577) - what a repeat-rich genome does to the index. */
int xm_index_bucket_stats(const xm_index* index, int64_t* buckets, int64_t* occupied, int64_t* overfull);
/* inspection (parity tests): one PackedMap as (counts per bucket or -1 if overfull, concatenated encoded positions) */
int xm_index_table_info(const xm_index* index, int32_t used_length, int32_t* capacity, int32_t* max_count_per_key, int64_t* num_stored, int64_t* num_overfull);
int xm_index_table_dump(const xm_index* index, int32_t used_length, int32_t* counts, int64_t* positions);
/* the PackedMap of one gapmer length: its keyCapacity and per-key limit (HashBlock_Database.java:569-577,620-665) without walking the buckets */
int xm_index_table_shape(const xm_index* index, int32_t used_length, int32_t* capacity, int32_t* max_count_per_key);
int64_t xm_index_dup_keys(const xm_index* index, int32_t contig, int32_t* out, int64_t cap);

/* Replaces the per-read loop of AlignerWorker.process() / Api.align (AlignerWorker.java:177-231,306-644): every query is
 * aligned on the GPU; *out is allocated by the library (its four streams are pinned host buffers from a pool the library keeps) and
 * released with xm_result_free.  Reads may contain IUPAC ambiguity codes (at most 128 ambiguous bases per mate).
 * A call fails as a whole - "Failed to align query q: the reference implementation would have thrown here" - when the reference would have thrown for one of
 * its queries: a mate contained in its partner (tryJoinQuerySequences asks for a range of negative length), a negative deviation, a deviation or expected
 * inner distance so large that the mate window wraps in 32-bit arithmetic (TreeMap.subMap: fromKey > toKey); INTEGRATION.md section 2 states the conditions.
 * q is the lowest failing query of the first pass that met one.  A call that fails leaves nothing behind: no result; nothing remembered
 * (xm_context_set_memo, xm_memory_new); no streams of a last call - xm_sam_format_last and xm_pileup_add_last fail with "no longer resident" after it,
 * whether or not an earlier call on the same resident batch had succeeded, until the next align call succeeds; the context's next call and the other
 * contexts of the index align as if it had not happened. */
int xm_align_batch(xm_index* index, const xm_params* params, const xm_query_batch* batch, xm_result** out);
void xm_result_free(xm_result* result);
/* The same in two steps, for callers that keep a batch in HBM (and for measuring the path without the PCIe copy):
 * xm_batch_upload validates and copies the batch to the device, xm_align_resident aligns the resident batch. */
int xm_batch_upload(xm_index* index, const xm_query_batch* batch);
int xm_align_resident(xm_index* index, const xm_params* params, xm_result** out);
/* The reference's workers take the next batch of queries while the previous one is being aligned (AlignerWorker.run / requestMoreWork,
 * AlignerWorker.java:92-175).  Here: xm_batch_stage copies the NEXT batch into a second set of device buffers on its own stream and may
 * run (from another host thread) while xm_align_resident is aligning the resident batch; xm_batch_commit then makes the staged batch
 * the resident one (it waits for a running xm_align_resident).  xm_batch_upload = stage + commit without the overlap.
 * (ABI version 8) xm_batch_unstage drops a staged batch that will not be committed - the batch behind one whose align call failed - so that a later
 * xm_batch_commit finds "no staged batch"; without a staged batch it does nothing.  The resident batch is untouched. */
int xm_batch_stage(xm_index* index, const xm_query_batch* batch);
int xm_batch_commit(xm_index* index);
int xm_batch_unstage(xm_index* index);

/* (ABI version 6) The batch staged from FASTQ text instead of from arrays: the host hands over a block of whole four-line records as it read them from the
 * file - one text for single reads, two texts of equally many records for pairs (record i of each is query i) - and kernels build the arrays of
 * xm_query_batch in HBM, so the host translates no base.  The texts may be pageable memory and are not needed after the call.  keep_qualities = 0: quals,
 * qual_off and has_qual of the result are NULL. */
typedef struct xm_fastq_text {
  const char* text1; int64_t bytes1; int64_t records1;
  const char* text2; int64_t bytes2; int64_t records2;   /* NULL / 0 / 0: single reads */
  double expected_inner, deviation;                       /* of every pair; single queries get 0 and 1 */
  int32_t keep_qualities;
  int32_t split_past_size;   /* (ABI version 12; was `reserved`, which callers set to 0)  0: a record is a query.  1 .. 30000: --split-queries-past-size on the GPU
                              * (SequenceSplitter.java:9-38) - the trimmed sequence of `length` bases becomes (length - 1) / split_past_size + 1 queries, section k
                              * being bases [length * k / n, length * (k + 1) / n) under the record's name, without quality (has_qual 0), its second slot
                              * the padding mate; a record may then be longer than 30000 bases.  Single reads only. */
} xm_fastq_text;
/* Host copies of what was built, in page-locked buffers of the library's pool: the fields of xmio_batch (include/xmapper_hostio.h) up to `store`, in its
 * order and with its meaning, so that the harness's writers read it as they read a batch of the host reader; then the times of the call's three parts. */
typedef struct xm_fastq_batch {
  int64_t num_queries; int32_t* mate_count; int64_t* mate_offset; int32_t* mate_length;
  uint8_t* codes; int64_t codes_length; char* names; int64_t* name_off;
  char* quals; int64_t* qual_off; uint8_t* has_qual; void* store;
  double h2d_ms, kernel_ms, d2h_ms;
} xm_fastq_batch;
/* Does what xm_batch_stage does (same stream, same buffers; xm_batch_commit follows as usual) and returns the arrays.  The device takes the strict form only:
 * every record is four lines, the first starts with '@', the sequence has 1 .. 30000 bases, and records1 / records2 are the records the texts hold (a last
 * line without its newline is a line).  Anything else fails the call with nothing staged; xm_last_error names the file (1 or 2), the 0-based record and
 * the reason.  A text may hold up to 1 GiB.  With split_past_size > 0 xm_fastq_batch.num_queries is the number of sections (the call waits for it once more,
 * to size what it builds per query), the 30000-base limit holds for a section instead of a record, errors still name the record, and text2 != NULL, a
 * negative size and one above 30000 are refused in the same way. */
int xm_batch_stage_fastq(xm_index* index, const xm_fastq_text* text, xm_fastq_batch** out);
void xm_fastq_batch_free(xm_fastq_batch* batch);
/* Bytes of text per workgroup of the kernels that find the line ends (test hook: tests/test_gpu_fastq.py puts newlines on both sides of the edges it gives). */
int32_t xm_fastq_tile_bytes(void);

/* (ABI version 12, added without a new version: look the symbol up)  The batch staged from FASTA text: what xm_batch_stage_fastq does for '>' records of any
 * number of lines.  A line is a header exactly when its first byte is '>'; every other line up to the next header belongs to the record, is trimmed of
 * blanks and tabs at both ends on its own and appended to the record's bases (so lines that start with '@', '+' or a blank are bases, as the host reader of
 * libxm_hostio.so has them).  The name is what stands behind '>' up to the first blank or tab.  records1 / lines1 (and records2 / lines2) are the headers and
 * the lines the texts hold, a last line without its newline being a line; a text holds at most 1 GiB and 2^26 lines.  A FASTA mate has no quality:
 * keep_qualities only sizes qual_off / has_qual as the host reader does (has_qual 0, quals empty).  split_past_size is xm_fastq_text's, for single reads. */
typedef struct xm_fasta_text {
  const char* text1; int64_t bytes1, records1, lines1;
  const char* text2; int64_t bytes2, records2, lines2;   /* NULL / 0 / 0 / 0: single reads */
  double expected_inner, deviation;                       /* of every pair; single queries get 0 and 1 */
  int32_t keep_qualities;
  int32_t split_past_size;
} xm_fasta_text;
/* The contract of xm_batch_stage_fastq, and its result (freed by xm_fastq_batch_free; the names belong to the staged batch, so xm_sam_format_last takes
 * names == NULL).  The strict form: the text's first byte is '>', the headers and lines found are the ones announced, every record has at least one base
 * and - without a split size - at most 30000; with one the limit holds for a section.  Anything else fails the call with nothing staged; xm_last_error
 * names the file (1 or 2), the 0-based record and the reason, the lowest (file, record) first. */
int xm_batch_stage_fasta(xm_index* index, const xm_fasta_text* text, xm_fastq_batch** out);

/* (ABI version 7) The SAM records of the last align call formatted on the GPU: the output-side counterpart of xm_batch_stage_fastq.  When an align call
 * returns, its four streams and its batch are still in HBM; kernels walk them there and build the text that the harness's host formatter
 * (xmio_write_batch, include/xmapper_hostio.h) builds from the copied streams, byte for byte: one line per sequence of every alignment, in query order, no
 * header.  The host is left with writing the bytes.  Not used by the Java host, which keeps its own writers.
 * xm_sam_set_contigs: the RNAME / RNEXT names, once per context, before the first format call; num_contigs must be the index's.
 * xm_sam_format_last has the contract of xm_pileup_add_last: it serialises with the context's other calls, runs on the context's stream, and fails with
 * "no longer resident" once another batch has been uploaded or committed, and after an align call that failed.  names == NULL: the names that xm_batch_stage_fastq built, which belong to the
 * batch in HBM (they change hands with it in xm_batch_commit); a batch that was staged from arrays has none, and the call fails.  Otherwise the mates'
 * names as xmio_batch holds them - name_off has 2 * num_queries + 1 entries, mate m of query q is names[name_off[2q + m] .. name_off[2q + m + 1]) - which
 * are copied up and may be pageable memory.  A slice that is not of the layout above (xmio_write_batch's "malformed result streams") fails the call with the
 * lowest such query in xm_last_error and no text.  *out: the text in a page-locked buffer of the library's pool (not NUL-terminated), its bytes and records
 * (lines), and the times of the call's three parts - names up, kernels, text down; released with xm_sam_text_free.  An unaligned query adds nothing. */
typedef struct xm_sam_names { const char* names; const int64_t* name_off; } xm_sam_names;
typedef struct xm_sam_text { char* text; int64_t bytes, records; double h2d_ms, kernel_ms, d2h_ms; void* store; } xm_sam_text;
int xm_sam_set_contigs(xm_index* context, int32_t num_contigs, const char* const* names);
int xm_sam_format_last(xm_index* context, const xm_sam_names* names, xm_sam_text** out);
void xm_sam_text_free(xm_sam_text* text);
/* Bytes of text per tile of the kernel that writes the records (test hook: tests/test_gpu_sam.py puts record ends on both sides of the multiples). */
int32_t xm_sam_tile_bytes(void);

/* (ABI version 10) The results left in HBM when only text and totals go to the host.  With xm_sam_format_last the host needs three small things of the four
 * streams: the statistics of Mapper.run (Mapper.java:786-796), the unaligned queries, and their number.  xm_summary_last computes them on the GPU from the
 * streams where they lie, and xm_context_set_result_copy(context, 0) then spares the copy of the streams altogether.  Not used by the Java host. */
/* default 1.  0: every later align call of this context leaves its four streams where they lie in HBM and copies none of them: the xm_result has
 * ints = dbls = int_off = dbl_off = NULL; num_queries, num_ints, num_dbls (the scan's totals: 16 bytes are read), counters, extra, the times and
 * kernel_launches are what they are with the copy.  The scan and gather launches are the same.  Per context; may be changed between calls. */
int xm_context_set_result_copy(xm_index* context, int32_t on);
/* What xmio_write_batch (include/xmapper_hostio.h) counts of a batch's streams when it writes no SAM: queries with an alignment, alignments, the sum of
 * lengthA over every block of every sequence, the blocks with lengthA != lengthB - and, because Mapper.run sums the penalties as doubles in query order and
 * the order is part of the result, the totalPenalty of every alignment in stream order for the host to add up (xmio_write_summary).  The arrays are
 * page-locked buffers of the library's pool (NULL where the count is 0); kernel_ms, d2h_ms: the kernels and the copy of the two arrays. */
typedef struct xm_batch_summary {
  int64_t num_queries, num_aligned, num_alignments, total_aligned_length, num_indels;
  int64_t num_unaligned; int64_t* unaligned;   /* ascending query indices; NULL / 0 when not asked for */
  double* penalties;                           /* [num_alignments]: totalPenalty of every alignment, stream order */
  double kernel_ms, d2h_ms; void* store;
} xm_batch_summary;
/* xm_summary_last has the contract of xm_pileup_add_last and xm_sam_format_last: it serialises with the context's other calls, runs on the context's stream,
 * and fails with "no longer resident" once another batch has been uploaded or committed, and after an align call that failed.  It works whether or not the
 * copy of the streams is on.  A slice that is not of the layout above - where xmio_write_batch without a SAM file reports "malformed result streams", and
 * also where a slice ends before the walk does - fails the call with the lowest such query in xm_last_error and no summary.  A batch of 0 queries launches
 * nothing and gives zeros.  Released with xm_summary_free.  mapper_amd/csrc/xm_summary_rules.h states the walk as code. */
int xm_summary_last(xm_index* context, int32_t want_unaligned, xm_batch_summary** out);
void xm_summary_free(xm_batch_summary* summary);

/* (no new ABI version: no struct or entry changed; a caller looks the two entries up by name, as xm_batch_stage_fasta)  The unaligned-query file written on
 * the GPU, and the staged batch kept in HBM.  A batch that xm_batch_stage_fastq / xm_batch_stage_fasta built from text comes back to the host whole - about as
 * many bytes as the text - and with xm_sam_format_last and xm_summary_last one reader of that copy is left: the harness's --out-unaligned, which rebuilds each
 * unaligned query's record from codes, names and qualities (xmio_write_summary).  xm_unaligned_format_last builds that text from the resident batch, and
 * xm_context_set_batch_copy(context, 0) then spares the copy.  Not used by the Java host.
 * xm_unaligned_format_last has xm_summary_last's contract: it serialises with the context's other calls, runs on the context's stream, fails with "no longer
 * resident" once another batch has been uploaded or committed and after an align call that failed, works whether or not the copy of the streams is on, and
 * fails with "malformed result streams: query N" for the lowest query whose slice is not of the layout (where xm_summary_last says so).  It fails for a batch
 * that was staged from arrays, which has no names in HBM.  The text: for every query without an alignment, in query order, each mate m < mate_count[q] as
 * xmio_write_batch writes it - '@' if the mate came as FASTQ and the batch was staged with keep_qualities, else '>'; the name; '\n'; the bases by code & 15
 * through ?ACMGRSVTWYHKDBN; '\n'; and for a FASTQ mate "+\n", the quality bytes, '\n' (mapper_amd/csrc/xm_unaligned_rules.h states it as code).  The
 * qualities belong to the batch in HBM as the names do: they change hands with it in xm_batch_commit, so staging the next block does not touch them.
 * *out: an xm_sam_text released with xm_sam_text_free - the text in a page-locked buffer (not NUL-terminated), its bytes, records = the mates written,
 * h2d_ms = 0, kernel_ms and d2h_ms the call's kernels and copy.  A batch of 0 queries launches nothing; a batch without an unaligned query gives bytes == 0
 * and launches nothing behind the totals.  Nothing is launched or allocated for a context that never calls it. */
int xm_unaligned_format_last(xm_index* context, xm_sam_text** out);
/* default 1.  0: every later xm_batch_stage_fastq / xm_batch_stage_fasta call of this context copies down only mate_count, mate_offset and mate_length (what
 * the host needs to know of the batch: the longest mate, any pair, the lengths); the returned xm_fastq_batch has codes = names = name_off = quals = qual_off =
 * has_qual = NULL and no pinned buffer is taken for them; num_queries, codes_length and the times are what they are.  keep_qualities still decides whether
 * the qualities are kept in HBM.  Per context; may be changed between calls. */
int xm_context_set_batch_copy(xm_index* context, int32_t on);

/* (ABI version 11) The queries of the last align call counted per combination of contigs - what Mapper.run's --out-refs-map-count reports
 * (Mapper.java:197, 747-756): for every query with an alignment, the set of contigs that the sequences of its alignments lie on, and per distinct set the
 * number of such queries.  Kernels walk the resident streams, find equal sets through a table keyed by a fingerprint of the set, compare every query's set
 * with its slot's first query, and count.  Between a few and a few thousand records cross to the host.  Not used by the Java host. */
#define XM_REFS_RECORD_IDS 8
typedef struct xm_refs_record {
  int64_t count;                /* queries with exactly this set */
  int32_t n;                    /* 1 .. XM_REFS_RECORD_IDS */
  int32_t ids[XM_REFS_RECORD_IDS];  /* ids[0 .. n): contig indices (reference order of the index), ascending and distinct; 0 behind them */
  int32_t reserved;
} xm_refs_record;
/* Every query with an alignment is either counted in one record or left over: a query on more than XM_REFS_RECORD_IDS contigs, or one whose set shares its
 * fingerprint with a different set (with 64 bits: practically never).  Of a left-over query the host gets the contig of every sequence alignment, repeats
 * included, in stream order: leftover_contigs[leftover_offsets[k] .. leftover_offsets[k + 1]) for the k-th of them in query order; the caller makes the set
 * and adds one to it.  The sets of two records differ.  sum(count) + num_leftover_queries == num_aligned.  The arrays are page-locked buffers of the
 * library's pool (NULL where the count is 0); kernel_ms, d2h_ms: the kernels and the copy of the arrays. */
typedef struct xm_refs_count {
  int64_t num_queries, num_aligned;
  int64_t num_combinations; xm_refs_record* records;
  int64_t num_leftover_queries; int64_t* leftover_offsets /* [num_leftover_queries + 1] */; int32_t* leftover_contigs;
  double kernel_ms, d2h_ms; void* store;
} xm_refs_count;
/* xm_refs_count_last has xm_summary_last's contract: it serialises with the context's other calls, runs on the context's stream, fails with "no longer
 * resident" once another batch has been uploaded or committed and after an align call that failed, works whether or not the copy of the streams is on, and
 * fails with "malformed result streams: query N" for the lowest query whose slice is not of the layout (where xm_summary_last says so).  Nothing is launched
 * or allocated for a context that never calls it, and a batch of 0 queries launches nothing.  Released with xm_refs_count_free.
 * mapper_amd/csrc/xm_refs_rules.h states the walk, the set and the fingerprint as code. */
int xm_refs_count_last(xm_index* context, xm_refs_count** out);
void xm_refs_count_free(xm_refs_count* count);

/* Bulk form of Readable_HashBlock_Database.getNumMatchesLowerBound + matchBlock / PackedMap.get (PackedMap.java:160-172,
 * 228-236) for n (used_length, lookup key) pairs: counts[i] = number of stored positions, -1 when the bucket is overfull or
 * holds more than the table's limit, -2 when used_length is not a hashed length.  Positions (at most max_per_probe <= 15 per probe, not reverse-complemented): the
 * probes of a chunk of 64 consecutive ones (i = 64c ... 64c + 63: a wavefront's) store theirs one behind the other, in probe order, from
 * out_positions[64c * max_per_probe] on; probe i's start within its chunk is the sum of min(max(counts[i'], 0), max_per_probe) over the chunk's probes
 * before it (out_positions holds n * max_per_probe entries; what no probe fills is not written).  Packed because the outputs are most of what such a
 * kernel moves: rows of max_per_probe slots would be 56 bytes a probe at 7 slots, of which a genome's buckets fill ~12.  Device-resident micro-kernel used for
 * the seed-lookup roofline measurement. */
int xm_seed_probe_packed(xm_index* index, int64_t n, const int32_t* used_length, const int32_t* keys, int32_t max_per_probe, int32_t* counts, int64_t* out_positions, double* kernel_ms);
/* (ABI version 2: this entry was xm_seed_probe with out_positions[j * n + i]; the packed layout has its own name so that a caller built against the old
 * header fails to link instead of reading garbage.  out_positions may be NULL: the kernel still fetches the positions - that is what is measured - and only
 * the counts are copied back.) */

/* Measurement helper for the seed-lookup roofline (SURVEY.md section 8d asks for the achieved rate next to "a measured random-64 B-gather
 * ceiling on the same GPU"): `accesses` reads of one random 64-byte sector each from a zero-filled device table of table_bytes;
 * kernel_ms = best of two timed launches.  No reference counterpart. */
int xm_measure_random_gather(int device, int64_t table_bytes, int64_t accesses, double* kernel_ms);

/* Pile-up of the alignments on the reference: what MatchDatabase.addAlignments / groupByPosition hand the
 * mutation and VCF writers (Mapper.java:700-708,758-785; behaviour pinned by MatchDatabase_Test.java:12-69 and MutationsWriter_Test.java:18-134).
 * xm_pileup_add_last accumulates, on the device, the alignments of the index's last xm_align_batch / xm_align_resident call (result streams and
 * batch still in HBM): per forward reference position the depth and the counts of differing query bases (A, C, G, T), in integer units of
 * 1 / XM_PILEUP_UNIT read bases (a query with n alignments adds 1/n per alignment; the mates of a pair add 1/2 each where they overlap), and one
 * event per insertion / deletion block: eight int64 = contig, position (startB of the block), type (1 insertion, 2 deletion), length, query
 * ordinal (over all batches added), mate | reversed << 1 | near-query-end << 2, startA, weight.  Several GPUs: one pile-up per replica, summed by the host in rank order.
 * The rules in full (tests/pileup_model.py recounts them on the host and the GPU tier compares the device with it, unit for unit):
 *  - weight: a component with n >= 1 alignments gives alignment a (0-based, stream order) UNIT / n, plus one unit when a < UNIT mod n, so the n weights
 *    sum to UNIT for any n (17, 19, 23 ... do not divide UNIT); a component without alignments adds nothing;
 *  - depth: every reference base under a block of equal lengths and every base of a deletion block (lengthA == 0) gets the weight; an insertion adds none;
 *  - alt: under a block of equal lengths the query base is the mate's base at startA + i on the strand that was aligned (the reverse complement of the
 *    mate as given when referenceReversed); it is counted in plane A, C, G or T only when it and the reference base are both unambiguous and differ;
 *  - mate: in a query with one component, sequence k of an alignment is mate k; with two components (the pair fell back to unpaired alignments)
 *    the sequences of component c are mate c;
 *  - overlap: the two sequences of one pair alignment that lie on the same contig share the depth where their reference intervals
 *    [first startB, last startB + lengthB) intersect: there the first adds w / 2 and the second w - w / 2 (integer division) - to depth, alt and middle
 *    alike; an event's weight is that of a base at its startB;
 *  - near a query end (fraction f > 0): query index k on the aligned strand with (double)k < f * len || (double)k >= len - f * len, len the mate's own
 *    length, evaluated in doubles as written; the bases of a deletion and every event take k = startA of their block;
 *  - the events of one xm_pileup_add_last call are ordered by (query ordinal, contig, position, flags, startA). */
#define XM_PILEUP_UNIT 1441440ull
typedef struct xm_pileup xm_pileup;
int xm_pileup_new(xm_index* index, xm_pileup** out);
/* MatchDatabase(queryEndFraction) (Mapper.java:76,351-353,700; --distinguish-query-ends, default 0.1 in Mapper.main): set before the first add.  With a
 * fraction > 0 the pile-up also keeps the "middle" depth - the depth from query bases that are not within that fraction of the query's length of
 * either query end - which is what the indel thresholds of the writers look at (Mapper.java:532-542, pinned by MutationsWriter_Test.java:114-134),
 * and events carry bit 2 of their flags word when they lie near a query end.  xm_pileup_read_middle reads it (fraction 0: equal to the depth). */
int xm_pileup_set_query_ends(xm_pileup* pileup, double fraction);
int xm_pileup_read_middle(xm_pileup* pileup, int32_t contig, int64_t first, int64_t n, uint64_t* depth);
int xm_pileup_add_last(xm_pileup* pileup, int64_t* num_events);
int xm_pileup_read(xm_pileup* pileup, int32_t contig, int64_t first, int64_t n, uint64_t* depth, uint64_t* alt /* [4][n] */);
int64_t xm_pileup_events(xm_pileup* pileup, int64_t first, int64_t n, int64_t* out /* [8 * n] */);
/* (ABI version 9) The text of the insertion events kept with them.  When an event is made its bases are in HBM with the batch; with on != 0 every later
 * xm_pileup_add_last also keeps them: kernels measure, place and write the letters of the call's insertions while the batch is resident, and the host copies
 * them down with the events and carries them through the same ordering, so that a caller needs the queries of no batch to write an insertion (the mutations
 * file: MutationsWriter_Test.java:18-134).  Off by default, and then xm_pileup_add_last launches and allocates what it did before; set before the first add.
 * The text of an insertion event: byte i is the letter (the 16 of QuickVariants Basepairs: ?ACMGRSVTWYHKDBN by code) of base startA + i of the event's mate
 * on the strand that was aligned - the complement of base readLen - 1 - (startA + i) of the mate as given when the reversed bit is set - for
 * i < min(length, readLen - startA), which is all of `length` for every event the library makes; a deletion event has no text.  The mate is bit 0 of the
 * flags word.  mapper_amd/csrc/xm_pileup_text_rules.h states this as code.
 * xm_pileup_event_text has xm_pileup_events' paging contract over the same events: text_off[0 .. m] are offsets into `text`, relative to the first byte
 * returned, event first + i owning [text_off[i], text_off[i + 1]); it returns m, the events served.  When text_cap bytes do not hold the text of all n
 * events it serves fewer - as many as fit, at least one; -1 when the first event alone does not fit, when first is outside of the events, and when text
 * was not kept.  Like the events the text is host memory: no live context and no GPU call are needed. */
int xm_pileup_keep_insert_text(xm_pileup* pileup, int32_t on);
int64_t xm_pileup_event_text(xm_pileup* pileup, int64_t first, int64_t n, int64_t* text_off /* [m + 1] */, char* text, int64_t text_cap);
void xm_pileup_free(xm_pileup* pileup);
/* (added without a new ABI version, as xm_unaligned_format_last was: no struct or entry changed; look them up by name)  The end of the mutations file on
 * the device: the counts stay where they are and only the answer crosses to the host - the SNP rows and, per indel candidate, a verdict.  The host path
 * (xm_pileup_read, xm_pileup_read_middle and the thresholds of mapper_amd/pileup.py) is the definition; mapper_amd/csrc/xm_mutations_rules.h states the rules as
 * the code the kernels run.  Not used by the Java host.  All three calls have xm_pileup_read's contract: they synchronise the device first, no
 * xm_pileup_add_last may run on the pile-up(s) meanwhile, and they need no live context.
 * The thresholds (MutationDetectionParameters [QuickVariants], Mapper.java:208-230): a pair (total depth, fraction) drops what it judges when the total depth
 * at the position is below the first, or when (float)support < (float)fraction * (float)total with the product taken in float32. */
typedef struct xm_mutation_filter {
  double min_snp_total_depth, min_indel_total_start_depth, min_indel_continuation_total_depth;
  float min_snp_depth_fraction, min_indel_start_depth_fraction, min_indel_continuation_depth_fraction;
  int32_t reserved;
} xm_mutation_filter;
/* xm_pileup_absorb moves the counts of `from` into `into`: into += from, from = 0, over depth, the four alt planes and the middle depth; the sum over both is
 * what it was, so xm_pileup_read over all pile-ups of a run gives the same sums before and after.  Events and kept insertion text stay with the pile-up that
 * collected them.  On one GPU it is one kernel; from another GPU, chunks come by peer copy into a buffer on into's GPU, are added there and cleared at the
 * source.  A `from` whose counts an earlier call moved away, and that no xm_pileup_add_last has added to since, holds zeros and is skipped.  Fails for a
 * null argument, the same handle twice, pile-ups of different indexes, different query-end fractions, and a `from` on a GPU that into's
 * GPU cannot reach by peer copy. */
int xm_pileup_absorb(xm_pileup* into, xm_pileup* from);
/* The SNP rows of the pile-up: one per (forward position, letter A, C, G, T by index 0..3) whose alt count is not 0 and passes the SNP pair over the depth at
 * the position; ordered by contig, position, letter.  Two passes over the counts and a scan over one count per XM_MUTATIONS_BLOCK positions
 * (xm_mutations_block_positions()); the rows come in a pinned buffer of the library (rows NULL when there are none - nothing is launched behind the total
 * then).  bytes_to_host: what the call copied to the host. */
typedef struct xm_snp_row {
  int32_t contig, position;              /* position: 0-based in the contig */
  uint8_t letter, reference_code, reserved[6];
  uint64_t support_units, total_units;   /* in units of 1 / XM_PILEUP_UNIT */
} xm_snp_row;
typedef struct xm_snp_calls {
  int64_t num_rows; xm_snp_row* rows;
  int64_t positions, bytes_to_host;
  double kernel_ms, d2h_ms;
  void* store;
} xm_snp_calls;
int xm_pileup_call_snps(xm_pileup* pileup, const xm_mutation_filter* filter, xm_snp_calls** out);
void xm_snp_calls_free(xm_snp_calls* calls);
int64_t xm_mutations_block_positions(void);
/* Indel candidates judged over the middle depth (the depth itself without a query-end fraction): candidate i = (contig, kind 1 insertion / 2 deletion, 1-based
 * pos1, length, support in units) gets verdicts[i] = (middle depth in units where it starts, keep), keep 0 when the start pair drops it, else 1 .. length: it
 * is cut in front of the first further base that the continuation pair drops (a deletion's bases where they lie, an insertion's all at its one position; no
 * position leaves the candidate's contig).  n = 0 launches nothing.  Fails for a contig outside of the reference or without bases, a kind other than 1 or 2. */
typedef struct xm_indel_candidate { int32_t contig, kind; int64_t pos1, length; uint64_t support_units; } xm_indel_candidate;
typedef struct xm_indel_verdict { uint64_t total_units; int64_t keep; } xm_indel_verdict;
int xm_pileup_judge_indels(xm_pileup* pileup, const xm_mutation_filter* filter, const xm_indel_candidate* candidates, int64_t n, xm_indel_verdict* verdicts);
/* (added without a new ABI version, like the entries above: look them up by name)  The insertion / deletion events grouped on the device as the batches come
 * in (mapper_amd/csrc/xm_indel_groups.h; the rules as code: xm_indel_groups_rules.h; the definition: MatchDatabase._indels() of mapper_amd/pileup.py).
 * xm_pileup_group_events(pileup, 1), before the first xm_pileup_add_last (it fails afterwards), makes every add fold the call's events into a table in HBM
 * that belongs to the pile-up and grows with it: a group is (contig, 1-based pos1, kind 1 insertion / 2 deletion, length, the insertion's letters) and its
 * support the sum of its events' weights; an insertion has pos1 = the event's position, a deletion pos1 = position + 1; events with bit 2 of their flags word
 * (near a query end) are in no group.  It implies xm_pileup_keep_insert_text - grouping needs the letters -, but neither events nor letters are copied to the
 * host any more, except those of LEFT-OVERS: events whose key met another key with the same 64-bit fingerprint in the table.  With grouping on,
 * xm_pileup_events, xm_pileup_event_text and xm_pileup_add_last's num_events speak of the left-overs only - in every run seen so far there are none -, and
 * the groups of the left-overs (the host makes them as ever) and the groups of the device's table of one pile-up are disjoint.
 * xm_pileup_call_indels judges the groups where they lie - xm_pileup_judge_indels' rule, over the middle depth - and returns those with keep > 0, each with
 * its letters at letters[letters_at .. letters_at + num_letters), in pinned buffers of the library; filter NULL: every group comes down unjudged, keep =
 * length, total_units as judged.  The order of the rows is not part of the contract.  xm_pileup_read's contract: it synchronises the device first and needs
 * no live context.  events: the events all adds made so far; groups: the groups of the table; left_over: the events the host holds; table_bytes: HBM of
 * the table, the records and the arena.  xm_pileup_absorb between two pile-ups that both group also folds from's groups into into's table and empties
 * from's; what that fold leaves over becomes events of `into` (query -1); it fails when only one of the two groups. */
typedef struct xm_indel_call {
  int32_t contig, kind;
  int64_t pos1, length, keep;
  uint64_t support_units, total_units;   /* in units of 1 / XM_PILEUP_UNIT */
  int64_t letters_at, num_letters;
} xm_indel_call;
typedef struct xm_indel_calls {
  int64_t num_rows; xm_indel_call* rows;
  int64_t num_letters; char* letters;
  int64_t groups, events, left_over, table_bytes, bytes_to_host;
  void* store;
} xm_indel_calls;
int xm_pileup_group_events(xm_pileup* pileup, int32_t on);
int xm_pileup_call_indels(xm_pileup* pileup, const xm_mutation_filter* filter, xm_indel_calls** out);
void xm_indel_calls_free(xm_indel_calls* calls);

/* TEST-ONLY entry (tests/test_gpu_kat.py; not part of the drop-in boundary): the reference's component-level known-answer tests run by the
 * device code of the align kernels over two given texts.  chain 0 = PathAligner alone (PathAligner_Test.java:10-39): mode 0 the lane-per-read
 * search in the wave's LDS slot, 1 the same search in HBM mode, 2 the wave-cooperative search with the search kernel's capacities, 3 with the
 * capacities of the chain tiers' inline searches, 4 the lane-private form of the search (xm_wsearch.h: what the chains of long reads and the reruns use).  chain 1 = HashBlock_Aligner -> StraightAligner -> PathAligner_Runner
 * (HashBlockAligner_Test.java:10-48): mode 0 searches slot-first as in the kernel, 1 all searches in HBM mode, 4 all in the lane-private form.
 * Returns 0 with blocks[4 * num_blocks] = (startA, startB, lengthA, lengthB) and penalties[2] = (total, aligned); 1 = no alignment (null); -1 = error. */
int xm_test_local_align(int32_t device, int32_t chain, int32_t mode, const xm_params* params, const uint8_t* query, int32_t query_length, const uint8_t* reference,
                        int32_t reference_length, double max_ins_ext, double max_del_ext, int32_t block_cap, int32_t* blocks, int32_t* num_blocks, double* penalties,
                        int64_t* nodes_put);
/* Test-only: what the rejection filter in front of PathAligner (mapper_amd/csrc/xm_bound.h) did in this thread's last xm_test_local_align call with mode + 8
 * (the search behind the filter): searches it took, searches it proved null, cells of its recurrence. */
void xm_test_bound_counters(int64_t* out3);
/* Test-only: the rejection filter alone on one problem - query[start_a, end_a) (query_rc: of the reverse complement of `query`) against
 * reference[start_b, end_b), the search's predictedBestOffset - run by one lane (pair: by the two lanes of a pair) of a wave, as the gapped passes of
 * long reads run it in front of PathAligner.align (PathAligner.java:55-293).  out3: 1 if the filter takes the problem, 1 if it proves the search null
 * (PathAligner.java:169), cells it computed.  tests/test_gpu_bound.py compares with the oracle's observer of the same bound, which also runs the search. */
int xm_test_bound(int32_t device, const xm_params* params, const uint8_t* query, int32_t query_length, int32_t query_rc, int32_t start_a, int32_t end_a, const uint8_t* reference,
                  int32_t reference_length, int32_t start_b, int32_t end_b, int32_t predicted_best_offset, int32_t pair, int64_t* out3);
/* Test-only (tests/test_gpu_sam.py): the kernels of xm_sam_format_last over host-given arrays - a batch with its names, contig names and the four result
 * streams - on `device`; no index and no alignment.  Same result, same errors. */
typedef struct xm_test_sam_job {
  int64_t num_queries; const int32_t* mate_count; const int64_t* mate_offset; const int32_t* mate_length; const uint8_t* codes; int64_t codes_length;
  const char* names; const int64_t* name_off;
  int32_t num_contigs, reserved; const char* const* contig_names;
  const int32_t* ints; const double* dbls; const int64_t* int_off; const int64_t* dbl_off;
} xm_test_sam_job;
int xm_test_sam_format(int32_t device, const xm_test_sam_job* job, xm_sam_text** out);
/* Test-only (tests/test_gpu_pileup_text.py): the kernels that keep the insertion text (xm_pileup_keep_insert_text) over host-given events - eight int64 each,
 * as xm_pileup_events returns them, holding anything - and the arrays of a batch, on `device`; no index and no alignment.  Query event[4] - query_base is the
 * event's.  text_off[num_events + 1] and the text as xm_pileup_event_text pages them, in the order of `events`; launches (may be NULL): kernels launched. */
typedef struct xm_test_pileup_job {
  int64_t num_queries; const int64_t* mate_offset; const int32_t* mate_length; const uint8_t* codes; int64_t codes_length;
  int64_t num_events; const int64_t* events; int64_t query_base;
} xm_test_pileup_job;
int xm_test_pileup_text(int32_t device, const xm_test_pileup_job* job, int64_t* text_off, char* text, int64_t text_cap, int32_t* launches);
/* Test-only (tests/test_gpu_summary.py), like xm_test_sam_format: the kernels of xm_summary_last over host-given streams on `device`; no index, no alignment.
 * Same result, same errors. */
int xm_test_summary(int32_t device, int64_t num_queries, int32_t num_contigs, const int32_t* ints, const double* dbls,
                    const int64_t* int_off, const int64_t* dbl_off, int32_t want_unaligned, xm_batch_summary** out);
/* Test-only (tests/test_gpu_unaligned.py), like xm_test_sam_format: the kernels of xm_unaligned_format_last over host-given arrays - a batch with its names,
 * its qualities (quals, qual_off and has_qual may all be NULL: a batch without them) and the four result streams - on `device`; no index and no alignment.
 * Same result, same errors.  The write kernel's tile is xm_sam_tile_bytes(). */
typedef struct xm_test_unaligned_job {
  int64_t num_queries; const int32_t* mate_count; const int64_t* mate_offset; const int32_t* mate_length; const uint8_t* codes; int64_t codes_length;
  const char* names; const int64_t* name_off;
  const char* quals; const int64_t* qual_off; const uint8_t* has_qual;
  int32_t num_contigs, reserved;
  const int32_t* ints; const double* dbls; const int64_t* int_off; const int64_t* dbl_off;
} xm_test_unaligned_job;
int xm_test_unaligned_format(int32_t device, const xm_test_unaligned_job* job, xm_sam_text** out);
/* Test-only (tests/test_gpu_refs_count.py), like xm_test_summary: the kernels of xm_refs_count_last over host-given streams on `device`; no index, no
 * alignment.  fingerprint_bits < 64 keeps only that many bits of the sets' fingerprints, so that different sets collide.  Same result, same errors. */
int xm_test_refs_count(int32_t device, int64_t num_queries, int32_t num_contigs, const int32_t* ints, const double* dbls,
                       const int64_t* int_off, const int64_t* dbl_off, int32_t fingerprint_bits, xm_refs_count** out);
/* Test-only (tests/test_gpu_mutations.py): the kernels of xm_pileup_absorb, xm_pileup_call_snps and xm_pileup_judge_indels over host-given counts on `device`; no
 * index, no alignment and no pile-up.  contig_lengths[num_contigs] (every one >= 1); one or two sets of counts in units - depth[total], alt[4][total] and
 * middle[total] (NULL in every set: the middle depth is the depth) -; with two sets the second is first absorbed into the first.  The rows (their
 * reference_code is 0: there is no reference) and the verdicts are those of set 0 afterwards; read_back[s] (may be NULL) receives set s as it then lies in HBM:
 * depth, the four alt planes and, when given, the middle depth, total entries each.  Same results, same errors. */
typedef struct xm_test_mutations_job {
  int32_t num_contigs, num_sets; const int32_t* contig_lengths;
  const uint64_t* depth[2]; const uint64_t* alt[2]; const uint64_t* middle[2];
  const xm_mutation_filter* filter;
  int64_t num_candidates; const xm_indel_candidate* candidates; xm_indel_verdict* verdicts;
  uint64_t* read_back[2];
} xm_test_mutations_job;
int xm_test_pileup_call(int32_t device, const xm_test_mutations_job* job, xm_snp_calls** out);
/* Test-only (tests/test_gpu_indel_groups.py): the kernels of xm_pileup_group_events over host-given events on `device`; no index, no alignment and no pile-up.
 * One or two sets of calls; a call is num_events events (eight int64 each, holding anything) with text_off[num_events + 1] into text, the letters of event i
 * at text[text_off[i] .. text_off[i + 1]).  Every set has a table of its own that starts with initial_capacity slots (rounded up to a power of two, at least
 * 4) and keeps fingerprint_bits bits of the fingerprints (64 and more: whole); with two sets the second is absorbed into the first after their calls.  out:
 * the groups of set 0 as xm_pileup_call_indels returns them with filter NULL (total_units 0: there are no counts).  The left-over events, at most left_cap
 * with at most left_text_cap letters, in the order the host holds them: left_events (eight int64 each), left_call (the call that left the event over: set 0's
 * calls count from 0, set 1's follow, the absorb comes last), left_text_off[num_left + 1] and left_text.  grows: how often the table, the records and the
 * arena of set 0 grew beyond their first allocation. */
typedef struct xm_test_group_call { int64_t num_events; const int64_t* events; const int64_t* text_off; const char* text; } xm_test_group_call;
typedef struct xm_test_group_job {
  int32_t fingerprint_bits, initial_capacity;
  int32_t num_calls[2]; const xm_test_group_call* calls[2];
  int64_t left_cap, left_text_cap;
  int64_t* left_events; int32_t* left_call; int64_t* left_text_off; char* left_text;
  int64_t num_left;
  int64_t grows[3];
} xm_test_group_job;
int xm_test_pileup_group(int32_t device, xm_test_group_job* job, xm_indel_calls** out);
/* Test-only (tests/test_gpu_scan.py): the exclusive prefix sums every on-GPU output stage takes (mapper_amd/csrc/xm_scan.h), alone, on `device`; no index and
 * no context.  lens: `channels` (1, 2 or 3) arrays of n lengths one behind the other; offsets: channels arrays of n + 1 sums the same way, the last of each
 * its total.  keep (may be NULL): n bytes, 0 or 1 - then kept[0 .. *num_kept) are the indices of the kept items in ascending order (kept holds n entries). */
int xm_test_scan(int32_t device, int32_t channels, int64_t n, const int64_t* lens, const uint8_t* keep, int64_t* offsets, int64_t* kept, int64_t* num_kept);
/* Test-only: Double.toString as the SAM tags print it, run by the device on n values: out24[24 * i ...] the string of x[i] (padded with NUL), len[i] its length. */
int xm_test_format_doubles(int32_t device, int64_t n, const double* x, char* out24, int32_t* len);

#ifdef __cplusplus
}
#endif
#endif
