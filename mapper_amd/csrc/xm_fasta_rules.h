// The rules of a FASTA record, once, as plain C++: what libxm_hostio.so's reader (xm_hostio.cpp, the FASTA branch of directMate and of
// nextRecord: the definition) makes of the lines of a '>' record, and the strict form, the part of what that reader accepts that the device parser takes.
// The kernels of xm_fasta.h call these functions on the device, the cutter of libxm_hostio.so (xmio_text_open_fasta) and tests/fasta_main.cpp call them on
// the host, so tests/test_fasta_text.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation.
//
// Lines are xm_fastq_rules.h's lines.  A line is a header exactly when its first byte - the raw one, nothing trimmed: the reader decides with peek() - is
// '>'; every other line behind a header is a body line of that header's record, up to the next header or the end of the text: empty lines, lines that start
// with '@', '+' or a blank (" >x" is body).  The name is the bytes behind '>' up to the first blank or tab (it may be empty).  A record's bases are its body
// lines, each trimmed on its own (fastqTrim), one behind the other; a blank inside a line stays and gets fastqCode's 15.
//
// Base ordinals: base b of a text is its b-th base in line order, a record is the range [first, first + length) of them, and section k of a record that is
// cut (fastqSectionCount, fastqSection, fastqSectionMate: unchanged) is a range of ordinals too.  baseBefore[line] - the exclusive scan of the lines' trimmed
// lengths, with baseBefore[lines] = the bases of the text - is the map from ordinals back to text positions (fastaLineOf).
#pragma once
#include "xm_fastq_rules.h"

namespace xm {

constexpr long long XM_FASTA_MAX_LINES = 1ll << 26;  // the lines of one text (a block of the cutter); at 60 columns that is 4 GiB, four times what a text may hold
constexpr int XM_FASTA_ORDINAL = 2;                  // in FastqMate::file beside the file's bit: seqAt is a base ordinal of that file, not a position in its text

// why a text is not of the strict form (0: it is); the lowest (file, record) of a batch is the one reported
enum FastaError : int {
  XM_FA_OK = 0,
  XM_FA_NO_HEADER = 1,   // the text's first byte is not '>' (the cutter drops a file's leading empty lines: a block starts at a header)
  XM_FA_NO_BASES = 2,    // a record of 0 bases: header after header, a header with nothing but empty or blank lines behind it, a header at the end of the text
  XM_FA_TOO_LONG = 3,    // without a split size: a record of more than XM_FASTQ_MAX_MATE bases
  XM_FA_RECORD_COUNT = 4,  // the headers found are not the records announced (an error of a file, not of a record)
  XM_FA_LINE_COUNT = 5     // the lines found are not the lines announced (an error of a file, not of a record)
};

inline const char* fastaErrorText(int e) {
  switch (e) {
    case XM_FA_NO_HEADER: return "the text does not start with a FASTA header ('>')";
    case XM_FA_NO_BASES:
    case XM_FA_TOO_LONG: return fastqErrorText(XM_FQ_TOO_LONG);  // validateBatch's words, as xm_fastq_rules.h has them
    case XM_FA_RECORD_COUNT: return "the text does not hold the FASTA records announced";
    case XM_FA_LINE_COUNT: return "the text does not hold the lines announced";
    default: return "no error";
  }
}

// the line [start, end) (end: the position of its '\n', or the text's size)
XM_FASTQ_FN bool fastaHeaderLine(const char* text, long long start, long long end) { return end > start && text[start] == '>'; }

// What a line gives: header -> true, [at, at + length) is the name; body -> false, [at, at + length) are its bases (trimmed; length may be 0).
XM_FASTQ_FN bool fastaLine(const char* text, long long start, long long end, long long& at, long long& length) {
  end = fastqLineEnd(text, start, end);
  if (fastaHeaderLine(text, start, end)) {
    long long k = start + 1;
    while (k < end && !fastqBlank(text[k])) k++;
    at = start + 1;
    length = k - (start + 1);
    return true;
  }
  fastqTrim(text, start, end);
  at = start;
  length = end - start;
  return false;
}
// the bases a line adds to the record it stands in (0 for a header)
XM_FASTQ_FN long long fastaLineBases(const char* text, long long start, long long end) {
  long long at, length;
  return fastaLine(text, start, end, at, length) ? 0 : length;
}

// a record of `length` bases (split = 0: it is a mate; split > 0: it is cut into sections of at most that many, so only an empty one is refused)
XM_FASTQ_FN int fastaRecordError(long long length, long long split) {
  if (length < 1) return XM_FA_NO_BASES;
  if (split == 0 && length > XM_FASTQ_MAX_MATE) return XM_FA_TOO_LONG;
  return XM_FA_OK;
}

// The line that holds base ordinal b (0 <= b < baseBefore[lines]): the last line with baseBefore[line] <= b, which has bases because the next one starts behind b.
template <class Int>
XM_FASTQ_FN long long fastaLineOf(const Int* baseBefore, long long lines, long long b) {
  long long lo = 0, hi = lines;  // baseBefore[lo] <= b < baseBefore[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)baseBefore[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace xm
