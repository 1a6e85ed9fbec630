/* libxm_hostio.so - host-side I/O of the standalone harness (python -m mapper_amd): FASTA / FASTQ in, SAM out, in native code.
 *
 * NOT part of the drop-in boundary (include/xmapper_hip.h is): in the drop-in deployment the Java host keeps reading the queries and writing the
 * SAM / VCF files (BASELINE.json north_star: "all I/O stays Java"; Mapper.java:699-732 hands every batch of QueryAlignments to its writers).  This
 * library exists so that the Python harness of SURVEY.md section 8(f) rank 1 can feed and drain a kernel that aligns millions of reads per second:
 * reads go from the file buffer to the flat batch arrays of xm_query_batch without an object per read, result streams go to SAM text without an
 * object per alignment.  Formats: what SamWriter_Test.java:18-94 pins, otherwise the SAM specification ([unpinned] in mapper_amd/sam.py, whose
 * records() xmio_write_batch reproduces byte for byte). */
#ifndef XMAPPER_HOSTIO_H
#define XMAPPER_HOSTIO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct xmio_reader xmio_reader;

/* One batch of queries: the arrays of xm_query_batch (mate 2 of a single query has length 0) + the names (one per mate: name_off[2 * q + m] ..
 * name_off[2 * q + m + 1] in `names`) and, when the reader keeps them, the quality strings the same way (has_qual[2 * q + m] = 1 for a FASTQ record). */
typedef struct xmio_batch {
  int64_t num_queries;
  const int32_t* mate_count;
  const int64_t* mate_offset;
  const int32_t* mate_length;
  const uint8_t* codes;
  int64_t codes_length;
  const char* names;
  const int64_t* name_off;   /* [2 * nq + 1] */
  const char* quals;         /* null unless the reader was opened with keep_qualities */
  const int64_t* qual_off;
  const uint8_t* has_qual;
  void* store;               /* owner of the arrays (xmio_batch_free) */
} xmio_batch;

/* Running totals of Mapper.run's statistics lines (Mapper.java:786-796), accumulated over the batches of a job in query order. */
typedef struct xmio_stats {
  int64_t num_queries, num_aligned, total_aligned_length, num_indels;
  double total_penalty;
} xmio_stats;

const char* xmio_last_error(void);
/* path2 != NULL: paired files read in step (a pair = one query).  split_past_size > 0: --split-queries-past-size (SequenceSplitter.java:9-38: a read longer
 * than that becomes equal sections, each a query of its own; single files only).  Files may be gzip-compressed. */
xmio_reader* xmio_open(const char* path1, const char* path2, int32_t split_past_size, int32_t keep_qualities);
/* The next up to max_queries queries; *out = NULL at the end of the input.  Returns 0, or -1 on a malformed file (xmio_last_error). */
int xmio_next(xmio_reader* reader, int64_t max_queries, xmio_batch** out);
void xmio_batch_free(xmio_batch* batch);
void xmio_close(xmio_reader* reader);
/* The result streams of `batch` (xm_result.ints / dbls / int_off / dbl_off) as SAM records (no header) to sam_fd and its unaligned queries (FASTQ when
 * they came with qualities, else FASTA) to unaligned_fd; either descriptor may be -1.  Query order; `threads` formatting threads.  Adds to *stats. */
int xmio_write_batch(const xmio_batch* batch, const int32_t* ints, const double* dbls, const int64_t* int_off, const int64_t* dbl_off, int32_t num_contigs,
                     const char* const* contig_names, int32_t sam_fd, int32_t unaligned_fd, int32_t threads, xmio_stats* stats);
/* xmio_write_batch with sam_fd = -1 for a caller that holds a summary of the streams instead of the streams (xm_batch_summary of include/xmapper_hip.h; the
 * SAM text is made and written elsewhere): the queries of `unaligned` - num_unaligned indices into the batch, strictly ascending, else the call fails and
 * writes nothing - go to unaligned_fd (-1: none) as xmio_write_batch writes them, and *stats grows by what xmio_write_batch would have added: the batch's
 * queries, the three counts, and total_penalty continued from its value by one += per entry of penalties[0 .. num_alignments), in order.  A batch whose
 * names or codes are NULL (it stayed in HBM: xm_context_set_batch_copy(0) of include/xmapper_hip.h) fails the call with a message when unaligned_fd >= 0 and
 * the list is not empty: the caller writes the text of xm_unaligned_format_last itself and passes unaligned_fd = -1. */
int xmio_write_summary(const xmio_batch* batch, int64_t num_aligned, int64_t total_aligned_length, int64_t num_indels, int64_t num_alignments,
                       const double* penalties, int64_t num_unaligned, const int64_t* unaligned, int32_t unaligned_fd, xmio_stats* stats);
/* Wall seconds of the calling thread's last xmio_write_batch or xmio_write_summary call: formatting and counting, and the write() calls (either may be NULL). */
void xmio_last_write_seconds(double* format_seconds, double* file_seconds);

/* The query files cut into blocks of whole four-line FASTQ records, as text, for a parser that is not this library's (xm_batch_stage_fastq of
 * include/xmapper_hip.h builds the batch arrays from such a block on the GPU).  The cutter looks for line ends only: no base is translated and nothing is
 * looked up per base.  Multi-line FASTQ records stay with xmio_open; FASTA records of any number of lines are cut by a reader opened with
 * xmio_text_open_fasta (for xm_batch_stage_fasta); --split-queries-past-size stays with xmio_open unless the reader is opened with xmio_text_open_split or
 * with xmio_text_open_fasta's split size, whose blocks go to a parser that cuts the sections (xm_fastq_text.split_past_size, xm_fasta_text.split_past_size). */
enum { XMIO_TEXT_FASTQ = 0, XMIO_TEXT_FASTA = 1 };
typedef struct xmio_text_reader xmio_text_reader;
typedef struct xmio_text_block {
  const char* text1; int64_t bytes1; int64_t records1;
  int64_t longest1;          /* length of the longest sequence line (lines 1, 5, 9, ...) of text1 as it stands in the file: an upper bound of the longest mate */
  const char* text2; int64_t bytes2; int64_t records2; int64_t longest2;   /* NULL / 0 / 0 / 0 for a single file */
  void* store;               /* owner of the texts (xmio_text_block_free) */
  int64_t num_queries;       /* (appended) the queries the block gives: records1, or - with a split size - the sections of its records, exactly */
  int64_t lines1, lines2;    /* (appended) the lines of each text, a last line without its newline included: 4 * records for FASTQ text */
  int32_t format;            /* (appended) XMIO_TEXT_FASTQ or XMIO_TEXT_FASTA: which parser the block is cut for */
} xmio_text_block;
/* path2 != NULL: paired files cut in step, a block holds the same number of records of each.  Files may be gzip-compressed. */
xmio_text_reader* xmio_text_open(const char* path1, const char* path2);
/* The next block: a contiguous copy of whole lines, at most max_queries records and at most 1 GiB per file; *out = NULL at the end of the input, where
 * trailing empty lines are dropped (the last block may lack its final newline).  Returns 0, or -1 (xmio_last_error names the file and the line) when a file
 * ends inside a record or the files of a pair hold different numbers of records. */
int xmio_text_next(xmio_text_reader* reader, int64_t max_queries, xmio_text_block** out);
/* One file whose records will be cut into sections of at most split_past_size (1 .. 30000) bases by the parser (SequenceSplitter.java:9-38, as xmio_open's
 * split_past_size does on the host).  A block is still whole records, but max_queries counts sections: per record the sequence line is trimmed at its ends
 * (fastqTrim of mapper_amd/csrc/xm_fastq_rules.h) and gives (length - 1) / split_past_size + 1 of them; the block stops in front of the record that would
 * pass max_queries and always takes at least one record, so a record of more sections than that is a block of its own.  longest1 is at most split_past_size.
 * Unlike xmio_next, no record's sections straddle two blocks. */
xmio_text_reader* xmio_text_open_split(const char* path, int32_t split_past_size);
/* One FASTA file, or two cut in step, for xm_batch_stage_fasta (the rules: mapper_amd/csrc/xm_fasta_rules.h).  A block is whole records: a record starts at a
 * line whose first byte is '>' and ends in front of the next such line or at the end of the input, so empty lines and lines that start with '@', '+' or a
 * blank belong to the record they stand in.  A file's leading empty lines are dropped; a first line that starts with neither '>' nor '@' is refused in the
 * host reader's words, and one that starts with '@' is refused as well.  max_queries counts records; with split_past_size (1 .. 30000, single file only; 0:
 * none) it counts sections, from the sum of the record's trimmed line lengths.  The block stops in front of the record that would pass max_queries, 1 GiB or
 * 2^26 lines, and always takes at least one record; a single record beyond 1 GiB or 2^26 lines is refused with its line.  longest1 / longest2 are the bases
 * of the longest record, capped at the split size.  Read through xmio_text_next; the blocks carry lines1 / lines2 and XMIO_TEXT_FASTA. */
xmio_text_reader* xmio_text_open_fasta(const char* path1, const char* path2, int32_t split_past_size);
/* The first byte of a query file's first line that is not empty ('>' or '@'; gzip is read through), 0 for a file of nothing but empty lines, -1 (xmio_last_error)
 * for a file that cannot be opened or whose first line starts with anything else: which cutter the file is for, without reading it twice. */
int xmio_first_header_byte(const char* path);
void xmio_text_block_free(xmio_text_block* block);
void xmio_text_close(xmio_text_reader* reader);

/* Double.toString(x) as the AS:f: / cs:f: tags print it (test hook); returns the length, -1 if cap is too small. */
int xmio_java_double(double x, char* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
