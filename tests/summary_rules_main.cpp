// The rules of the batch summary (mapper_amd/csrc/xm_summary_rules.h: plain C++ that the kernels of xm_summary.h call) run on the host, for
// tests/test_summary_rules.py, which builds this file with g++ (with -fsanitize=address,undefined where the host compiler has the runtime).
//   summary_rules_main walk FILE   the walk over every query of the case: "ok nq aligned alignments length indels", then the alignments per query, the
//                                  unaligned queries and the penalties as bit patterns, a line each; or "malformed Q" with the lowest malformed query
//   summary_rules_main cut FILE    a case of one query: its slice cut short at every position, each cut in a heap block of its own size (a read behind
//                                  the cut is a read behind the block: the sanitizer build stops there), must be malformed
// FILE: int64 head[4] = queries, ints, doubles, contigs; then ints, dbls, int_off[nq + 1], dbl_off[nq + 1] (tests/summary_cases.py write_streams).
#include "../mapper_amd/csrc/xm_summary_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Case {
  int64_t head[4] = {0, 0, 0, 0};
  std::vector<int32_t> ints;
  std::vector<double> dbls;
  std::vector<int64_t> intOff, dblOff;
  template <class T> static void take(FILE* f, std::vector<T>& v, int64_t n) {
    if (n < 0) { fprintf(stderr, "negative size\n"); exit(2); }
    v.resize((size_t)n);
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "case file too short\n"); exit(2); }
  }
  explicit Case(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f || fread(head, sizeof(int64_t), 4, f) != 4) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    take(f, ints, head[1]); take(f, dbls, head[2]); take(f, intOff, head[0] + 1); take(f, dblOff, head[0] + 1);
    fclose(f);
  }
  xm::SummaryStreams streams() const { return xm::SummaryStreams{ints.data(), dbls.data(), intOff.data(), dblOff.data(), (int32_t)head[3]}; }
};

struct PenaltyList {
  std::vector<double> all;
  long long first = 0;  // alignments of the queries before this one
  bool inOrder = true;
  void penalty(long long a, double p) {
    if (first + a != (long long)all.size()) inOrder = false;
    all.push_back(p);
  }
};

int walk(const char* path) {
  const Case c(path);
  const xm::SummaryStreams st = c.streams();
  const int64_t nq = c.head[0];
  long long aligned = 0, length = 0, indels = 0;
  std::vector<long long> perQuery;
  std::vector<long long> unaligned;
  PenaltyList list;
  for (int64_t q = 0; q < nq; q++) {
    xm::QuerySummary counted, s;
    xm::SummaryNoPenalties none;
    if (!xm::summaryWalkQuery(st, q, counted, none)) { printf("malformed %lld\n", (long long)q); return 0; }
    list.first = (long long)list.all.size();
    if (!xm::summaryWalkQuery(st, q, s, list)) { printf("malformed %lld\n", (long long)q); return 0; }
    if (s.alignments != counted.alignments || s.aligned != counted.aligned || s.alignedLength != counted.alignedLength || s.indels != counted.indels ||
        (long long)list.all.size() - list.first != s.alignments || !list.inOrder) {
      fprintf(stderr, "query %lld: the two walks differ\n", (long long)q);
      return 3;
    }
    aligned += s.aligned; length += s.alignedLength; indels += s.indels;
    perQuery.push_back(s.alignments);
    if (!s.aligned) unaligned.push_back(q);
  }
  printf("ok %lld %lld %zu %lld %lld\n", (long long)nq, aligned, list.all.size(), length, indels);
  for (long long n : perQuery) printf("%lld ", n);
  printf("\n");
  for (long long q : unaligned) printf("%lld ", q);
  printf("\n");
  for (double p : list.all) { uint64_t bits; memcpy(&bits, &p, 8); printf("%016llx ", (unsigned long long)bits); }
  printf("\n");
  return 0;
}

int cut(const char* path) {
  const Case c(path);
  if (c.head[0] != 1) { fprintf(stderr, "cut takes a case of one query\n"); return 2; }
  const int64_t ni = (int64_t)c.ints.size(), nd = (int64_t)c.dbls.size();
  for (int64_t len = 0; len <= ni; len++) {
    int32_t* ints = new int32_t[(size_t)len];
    if (len) memcpy(ints, c.ints.data(), sizeof(int32_t) * (size_t)len);
    const int64_t intOff[2] = {0, len};
    const xm::SummaryStreams st{ints, c.dbls.data(), intOff, c.dblOff.data(), (int32_t)c.head[3]};
    xm::QuerySummary s;
    xm::SummaryNoPenalties none;
    const bool ok = xm::summaryWalkQuery(st, 0, s, none);
    delete[] ints;
    if (ok != (len == ni)) { printf("cut ints %lld of %lld: %s\n", (long long)len, (long long)ni, ok ? "accepted" : "malformed"); return 0; }
  }
  for (int64_t len = 0; len < nd; len++) {
    double* dbls = new double[(size_t)len];
    if (len) memcpy(dbls, c.dbls.data(), sizeof(double) * (size_t)len);
    const int64_t dblOff[2] = {0, len};
    const xm::SummaryStreams st{c.ints.data(), dbls, c.intOff.data(), dblOff, (int32_t)c.head[3]};
    xm::QuerySummary s;
    xm::SummaryNoPenalties none;
    const bool ok = xm::summaryWalkQuery(st, 0, s, none);
    delete[] dbls;
    if (ok) { printf("cut dbls %lld of %lld: accepted\n", (long long)len, (long long)nd); return 0; }
  }
  printf("cut ok %lld %lld\n", (long long)ni, (long long)nd);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "walk") && argc > 2) return walk(argv[2]);
  if (!strcmp(mode, "cut") && argc > 2) return cut(argv[2]);
  fprintf(stderr, "usage: summary_rules_main walk FILE | cut FILE\n");
  return 2;
}
