// The rules of the unaligned-query file's text (mapper_amd/csrc/xm_unaligned_rules.h over xm_summary_rules.h: plain C++ that the kernels of xm_unaligned.h
// call) run on the host, for tests/test_unaligned_rules.py, which builds this file with g++ (with -fsanitize=address,undefined where the host compiler has the
// runtime).  The four stages of xm_unaligned.h with one thread:
//   measure   per query the unaligned flag (summaryWalkQuery) and the record's bytes (unalignedRecordBytes); the lowest malformed query ends the run
//   offsets   exclusive sums of both arrays
//   compact   the ascending list of the unaligned queries
//   write     per list entry the record into its own range of a heap block of exactly the text's size (a byte outside the range is an error, and one
//             outside the block is the sanitizer's to find)
//   unaligned_rules_main format FILE   "ok BYTES MATES UNALIGNED\n" and the text behind it; or "malformed Q\n" with the lowest malformed query
// FILE: int64 head[8] = queries, codes, name bytes, quality bytes, has_qual given (0 / 1), ints, doubles, contigs; then mate_count, mate_offset[2 nq],
// mate_length[2 nq], codes, names, name_off[2 nq + 1], (quals, qual_off[2 nq + 1], has_qual[2 nq] when given), ints, dbls, int_off[nq + 1], dbl_off[nq + 1]
// (tests/unaligned_cases.py write_case).
#include "../mapper_amd/csrc/xm_summary_rules.h"
#include "../mapper_amd/csrc/xm_unaligned_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

template <class T> void take(FILE* f, std::vector<T>& v, int64_t n) {
  if (n < 0) { fprintf(stderr, "negative size\n"); exit(2); }
  v.resize((size_t)n);
  if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "case file too short\n"); exit(2); }
}

struct Case {
  int64_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int32_t> mateCount, mateLength, ints;
  std::vector<int64_t> mateOffset, nameOff, qualOff, intOff, dblOff;
  std::vector<uint8_t> codes, hasQual;
  std::vector<char> names, quals;
  std::vector<double> dbls;
  explicit Case(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f || fread(head, sizeof(int64_t), 8, f) != 8) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    const int64_t nq = head[0];
    take(f, mateCount, nq); take(f, mateOffset, 2 * nq); take(f, mateLength, 2 * nq); take(f, codes, head[1]); take(f, names, head[2]); take(f, nameOff, 2 * nq + 1);
    if (head[4]) { take(f, quals, head[3]); take(f, qualOff, 2 * nq + 1); take(f, hasQual, 2 * nq); }
    take(f, ints, head[5]); take(f, dbls, head[6]); take(f, intOff, nq + 1); take(f, dblOff, nq + 1);
    fclose(f);
  }
  xm::UnalignedBatch batch() const {
    const bool q = head[4] != 0;
    return xm::UnalignedBatch{head[0], mateCount.data(), mateOffset.data(), mateLength.data(), codes.data(), head[1], names.data(), nameOff.data(), head[2],
                              q ? quals.data() : nullptr, q ? qualOff.data() : nullptr, q ? hasQual.data() : nullptr, q ? head[3] : 0};
  }
  xm::SummaryStreams streams() const { return xm::SummaryStreams{ints.data(), dbls.data(), intOff.data(), dblOff.data(), (int32_t)head[7]}; }
};

// the sink of the write stage: bytes go to text[at], which must stay inside [lo, hi)
struct RangeSink {
  char* text;
  long long lo, hi, at;
  bool inside = true;
  void put(char c) {
    if (at < lo || at >= hi) inside = false; else text[at] = c;
    at++;
  }
  template <class F> void compose(F f) {
    char room[xm::XM_UNALIGNED_ROOM];
    const int n = f(room);
    if (n < 0 || n > xm::XM_UNALIGNED_ROOM) { inside = false; return; }
    for (int i = 0; i < n; i++) put(room[i]);
  }
  template <class G> void spread(long long n, G byteAt) {
    for (long long i = 0; i < n; i++) put(byteAt(i));
  }
};

int format(const char* path) {
  const Case c(path);
  const xm::UnalignedBatch b = c.batch();
  const xm::SummaryStreams st = c.streams();
  const int64_t nq = c.head[0];
  // measure
  std::vector<long long> bytes((size_t)nq, 0), flag((size_t)nq, 0);
  long long mates = 0;
  for (int64_t q = 0; q < nq; q++) {
    xm::QuerySummary s;
    xm::SummaryNoPenalties none;
    if (!xm::summaryWalkQuery(st, q, s, none)) { printf("malformed %lld\n", (long long)q); return 0; }
    if (!s.aligned) { flag[(size_t)q] = 1; bytes[(size_t)q] = xm::unalignedRecordBytes(b, q); mates += xm::unalignedMates(b, q); }
  }
  // offsets
  std::vector<long long> off((size_t)nq + 1, 0), uoff((size_t)nq + 1, 0);
  for (int64_t q = 0; q < nq; q++) { off[(size_t)q + 1] = off[(size_t)q] + bytes[(size_t)q]; uoff[(size_t)q + 1] = uoff[(size_t)q] + flag[(size_t)q]; }
  const long long total = off[(size_t)nq], unaligned = uoff[(size_t)nq];
  // compact
  std::vector<long long> list((size_t)unaligned, -1);
  for (int64_t q = 0; q < nq; q++) if (uoff[(size_t)q + 1] > uoff[(size_t)q]) list[(size_t)uoff[(size_t)q]] = q;
  // write
  char* text = new char[(size_t)total];
  memset(text, '#', (size_t)total);
  long long written = 0;
  for (long long i = 0; i < unaligned; i++) {
    const long long q = list[(size_t)i];
    if (q < 0 || q >= nq || (i > 0 && q <= list[(size_t)i - 1])) { fprintf(stderr, "the list is not ascending at entry %lld\n", i); return 3; }
    RangeSink sink{text, off[(size_t)q], off[(size_t)q + 1], off[(size_t)q]};
    written += xm::unalignedWriteQuery(b, q, sink);
    if (!sink.inside || sink.at != sink.hi) { fprintf(stderr, "query %lld: the record did not end where it was measured to\n", q); return 3; }
  }
  if (written != mates) { fprintf(stderr, "the mates written differ from the mates measured\n"); return 3; }
  printf("ok %lld %lld %lld\n", total, mates, unaligned);
  if (total) fwrite(text, 1, (size_t)total, stdout);
  delete[] text;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "format") && argc > 2) return format(argv[2]);
  fprintf(stderr, "usage: unaligned_rules_main format FILE\n");
  return 2;
}
