// The rules of a four-line FASTQ record, once, as plain C++: what libxm_hostio.so's reader (xm_hostio.cpp, directMate: the definition)
// makes of the lines of a record - where a line ends, what the name is, how the sequence and the quality are trimmed, which code a base gets - and the
// strict form, the part of what that reader accepts that the device parser takes.  The kernels of xm_fastq.h call these functions on the device (they are
// host+device there, and plain inline functions everywhere else), the cutter of libxm_hostio.so (xmio_text_next) and tests/fastq_rules_main.cpp call them
// on the host, so tests/test_fastq_text.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation.
//
// A text is `bytes` bytes.  Line k ends at the k-th '\n' (its position is the line's end; the next line starts one behind it); a text whose last byte is
// not '\n' has one more line, ending at `bytes` (only the last block of a file may look like that).  One '\r' in front of the line's end is not part of the line.
// Record r is lines 4r .. 4r + 3: header, sequence, plus line (never looked at), quality.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_FASTQ_FN __host__ __device__ __forceinline__
#else
#define XM_FASTQ_FN inline
#endif

namespace xm {

constexpr int XM_FASTQ_MAX_MATE = 30000;  // the longest mate a batch may hold (xm_capi.hip, validateBatch)

// why a record is not of the strict form (0: it is); the lowest (file, record) of a batch is the one reported
enum FastqError : int {
  XM_FQ_OK = 0,
  XM_FQ_EMPTY_HEADER = 1,  // an empty line where a header is expected (the host reader skips it)
  XM_FQ_FASTA = 2,         // a '>' record (the host reader takes it)
  XM_FQ_NO_HEADER = 3,     // any other first byte (the host reader refuses it too)
  XM_FQ_NO_BASES = 4,      // a sequence of length 0
  XM_FQ_TOO_LONG = 5,      // a sequence of more than XM_FASTQ_MAX_MATE bases
  XM_FQ_LINE_COUNT = 6     // the text does not hold four lines per record (FastqError of a file, not of a record)
};

inline const char* fastqErrorText(int e) {
  switch (e) {
    case XM_FQ_EMPTY_HEADER: return "an empty line where a FASTQ header is expected";
    case XM_FQ_FASTA: return "a FASTA record ('>'), the device parser takes four-line FASTQ records only";
    case XM_FQ_NO_HEADER: return "the record's first line does not start with '@'";
    case XM_FQ_NO_BASES:
    case XM_FQ_TOO_LONG: return "mate length out of range (1..30000; longer reads are split by the caller as --split-queries-past-size does)";
    case XM_FQ_LINE_COUNT: return "the text does not hold four lines per record";
    default: return "no error";
  }
}

// g_code of xm_hostio.cpp: ACGTURYSWKMBDHVN in either case -> 1 2 4 8 8 5 10 6 9 12 3 14 13 11 7 15, every other byte (bytes >= 128 included) -> 15
XM_FASTQ_FN uint8_t fastqCode(unsigned char c) {
  switch (c | 0x20) {  // (only a letter becomes a lower-case letter by this)
    case 'a': return 1;
    case 'c': return 2;
    case 'g': return 4;
    case 't': return 8;
    case 'u': return 8;
    case 'r': return 5;
    case 'y': return 10;
    case 's': return 6;
    case 'w': return 9;
    case 'k': return 12;
    case 'm': return 3;
    case 'b': return 14;
    case 'd': return 13;
    case 'h': return 11;
    case 'v': return 7;
    default: return 15;
  }
}

XM_FASTQ_FN bool fastqBlank(char c) { return c == ' ' || c == '\t'; }

// [start, end) of a line without its terminator: `end` is the position of its '\n' (or `bytes`); one '\r' in front of it goes
XM_FASTQ_FN long long fastqLineEnd(const char* text, long long start, long long end) { return end > start && text[end - 1] == '\r' ? end - 1 : end; }

// the sequence and the quality line: blanks and tabs trimmed in front; blanks, tabs and '\r' trimmed behind
XM_FASTQ_FN void fastqTrim(const char* text, long long& start, long long& end) {
  while (end > start && fastqBlank(text[start])) start++;
  while (end > start && (fastqBlank(text[end - 1]) || text[end - 1] == '\r')) end--;
}

// what a record is made of: positions in its file's text
struct FastqFields {
  long long nameAt, seqAt, qualAt;
  long long nameLen, seqLen, qualLen;
};

// The record whose four lines are [s0, e0) .. [s3, e3) (each e the position of the line's '\n', or `bytes`) -> its fields, or why it is not of the strict form.
XM_FASTQ_FN int fastqRecord(const char* text, long long s0, long long e0, long long s1, long long e1, long long s3, long long e3, FastqFields& f) {
  f.nameAt = f.seqAt = f.qualAt = s0;
  f.nameLen = f.seqLen = f.qualLen = 0;
  e0 = fastqLineEnd(text, s0, e0);
  if (e0 == s0) return XM_FQ_EMPTY_HEADER;
  if (text[s0] == '>') return XM_FQ_FASTA;
  if (text[s0] != '@') return XM_FQ_NO_HEADER;
  long long k = s0 + 1;  // the name: behind '@' up to the first blank or tab (it may be empty)
  while (k < e0 && !fastqBlank(text[k])) k++;
  f.nameAt = s0 + 1;
  f.nameLen = k - (s0 + 1);
  e1 = fastqLineEnd(text, s1, e1);
  fastqTrim(text, s1, e1);
  f.seqAt = s1;
  f.seqLen = e1 - s1;
  e3 = fastqLineEnd(text, s3, e3);
  fastqTrim(text, s3, e3);
  f.qualAt = s3;
  f.qualLen = e3 - s3;
  if (f.seqLen < 1) return XM_FQ_NO_BASES;
  if (f.seqLen > XM_FASTQ_MAX_MATE) return XM_FQ_TOO_LONG;
  return XM_FQ_OK;
}

// ---- the split form (--split-queries-past-size): a record of a single file becomes the sections SequenceSplitter.java:9-38 cuts it into, each a
// query of its own.  The definitions are the split branch of xmio_next (xm_hostio.cpp) and cli.split_sections.
// sections of a sequence of `length` >= 1 bases cut past `split` >= 1 bases
XM_FASTQ_FN long long fastqSectionCount(long long length, long long split) { return (length - 1) / split + 1; }
// section k of `count`: [length * k / count, length * (k + 1) / count) in 64-bit integers (length and count below 2^31: no product overflows)
XM_FASTQ_FN void fastqSection(long long length, long long count, long long k, long long& start, long long& end) {
  start = length * k / count;
  end = length * (k + 1) / count;
}
// fastqRecord for a record that will be cut: its sequence - trimmed first, as the host reader trims it - may be as long as the text allows; every other
// refusal stays.  What it leaves in f.qual* is not used: a section has no quality.
XM_FASTQ_FN int fastqRecordSplit(const char* text, long long s0, long long e0, long long s1, long long e1, long long s3, long long e3, FastqFields& f) {
  const int err = fastqRecord(text, s0, e0, s1, e1, s3, e3, f);  // (the length is the last thing it looks at: the fields of a record that is too long are complete)
  return err == XM_FQ_TOO_LONG ? XM_FQ_OK : err;
}
// section k of the `count` of record `rec` as the mate of its query's first slot: the record's name, its slice of the sequence, no quality (has_qual 0);
// the query's second slot is the padding mate
XM_FASTQ_FN void fastqSectionMate(const FastqFields& rec, long long count, long long k, FastqFields& m) {
  long long start, end;
  fastqSection(rec.seqLen, count, k, start, end);
  m.nameAt = rec.nameAt; m.nameLen = rec.nameLen;
  m.seqAt = rec.seqAt + start; m.seqLen = end - start;
  m.qualAt = rec.seqAt; m.qualLen = 0;
}
// the sequence line [start, end) of a record (end: the position of its '\n', or the text's size) -> its sections; 0 for a line that trims to nothing (the
// parser refuses the record).  The cutter of libxm_hostio.so counts a block's queries with this: it looks at the ends of the line only.
XM_FASTQ_FN long long fastqLineSections(const char* text, long long start, long long end, long long split) {
  end = fastqLineEnd(text, start, end);
  fastqTrim(text, start, end);
  return end > start ? fastqSectionCount(end - start, split) : 0;
}

// Batch order: query i is record i of file 1 and, for pairs, record i of file 2 as its second mate; a query has two mate slots, 2i and 2i + 1.  The second
// slot of a single query is the padding mate: offset 0, length 0, no name, no quality, has_qual 0.  Every real mate has has_qual 1.
XM_FASTQ_FN long long fastqMateSlot(long long record, int file) { return 2 * record + file; }
XM_FASTQ_FN bool fastqPaddingMate(long long slot, bool paired) { return !paired && (slot & 1) != 0; }

// a line is empty when nothing is left of it without its '\r' (the reader skips such lines in front of a header; at the end of a file the cutter drops them)
XM_FASTQ_FN bool fastqEmptyLine(const char* text, long long start, long long end) { return fastqLineEnd(text, start, end) == start; }

}  // namespace xm
