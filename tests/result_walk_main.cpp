// The three visitors of the result walk (mapper_amd/csrc/xm_result_walk.h) - the SAM records, the summary and the reference sets - run side by side on the
// host over the same slices, for tests/test_result_walk.py, which builds this file with g++ (with -fsanitize=address,undefined where the host compiler has
// the runtime) and compares their verdicts.
//   result_walk_main verdicts FILE   a line "S U R" per query: 1 where the SAM walk, the summary's and the reference sets' take the slice, 0 where malformed
//   result_walk_main cuts FILE       a case of one query: its slice cut short at every position of the int stream ("i LEN S U R") and of the doubles
//                                    ("d LEN S U R"), each cut in a heap block of its own size (a read behind the cut is a read behind the block)
// FILE: tests/sam_cases.py write_case.
#include "../mapper_amd/csrc/xm_refs_rules.h"
#include "../mapper_amd/csrc/xm_sam_rules.h"
#include "../mapper_amd/csrc/xm_summary_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Case {
  int64_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // queries, codes, name bytes, ints, doubles, contigs, contig name bytes, 0
  std::vector<int32_t> mateCount, mateLength, ints;
  std::vector<int64_t> mateOffset, nameOff, intOff, dblOff, contigOff;
  std::vector<uint8_t> codes;
  std::vector<char> names, contigNames;
  std::vector<double> dbls;
  template <class T> static void take(FILE* f, std::vector<T>& v, int64_t n) {
    if (n < 0) { fprintf(stderr, "negative size\n"); exit(2); }
    v.resize((size_t)n);
    if (n && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "case file too short\n"); exit(2); }
  }
  explicit Case(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f || fread(head, sizeof(int64_t), 8, f) != 8) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    const int64_t nq = head[0];
    take(f, mateCount, nq); take(f, mateOffset, 2 * nq); take(f, mateLength, 2 * nq); take(f, codes, head[1]); take(f, names, head[2]); take(f, nameOff, 2 * nq + 1);
    take(f, ints, head[3]); take(f, dbls, head[4]); take(f, intOff, nq + 1); take(f, dblOff, nq + 1); take(f, contigNames, head[6]); take(f, contigOff, head[5] + 1);
    fclose(f);
  }
  xm::SamBatch batch() const { return xm::SamBatch{head[0], mateCount.data(), mateOffset.data(), mateLength.data(), codes.data(), names.data(), nameOff.data()}; }
  xm::SamContigs contigs() const { return xm::SamContigs{(int32_t)head[5], contigNames.data(), contigOff.data()}; }
};

// "S U R" for query q of the streams
void verdicts(const Case& c, const xm::ResultStreams& st, long long q) {
  const xm::SamBatch b = c.batch();
  const xm::SamContigs contigs = c.contigs();
  xm::SamCount count;
  xm::QuerySummary summary;
  xm::SummaryNoPenalties none;
  xm::RefSet set;
  const bool s = xm::samWalkQuery(b, st, contigs, q, count), u = xm::summaryWalkQuery(st, q, summary, none), r = xm::refsWalkQuery(st, q, set);
  printf("%d %d %d\n", s ? 1 : 0, u ? 1 : 0, r ? 1 : 0);
}

int all(const char* path) {
  const Case c(path);
  const xm::ResultStreams st{c.ints.data(), c.dbls.data(), c.intOff.data(), c.dblOff.data(), (int32_t)c.head[5]};
  for (int64_t q = 0; q < c.head[0]; q++) verdicts(c, st, q);
  return 0;
}

int cuts(const char* path) {
  const Case c(path);
  if (c.head[0] != 1) { fprintf(stderr, "cuts takes a case of one query\n"); return 2; }
  const int64_t ni = (int64_t)c.ints.size(), nd = (int64_t)c.dbls.size();
  for (int64_t len = 0; len <= ni; len++) {
    int32_t* ints = new int32_t[(size_t)len];
    if (len) memcpy(ints, c.ints.data(), sizeof(int32_t) * (size_t)len);
    const int64_t intOff[2] = {0, len};
    printf("i %lld ", (long long)len);
    verdicts(c, xm::ResultStreams{ints, c.dbls.data(), intOff, c.dblOff.data(), (int32_t)c.head[5]}, 0);
    delete[] ints;
  }
  for (int64_t len = 0; len <= nd; len++) {
    double* dbls = new double[(size_t)len];
    if (len) memcpy(dbls, c.dbls.data(), sizeof(double) * (size_t)len);
    const int64_t dblOff[2] = {0, len};
    printf("d %lld ", (long long)len);
    verdicts(c, xm::ResultStreams{c.ints.data(), dbls, c.intOff.data(), dblOff, (int32_t)c.head[5]}, 0);
    delete[] dbls;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "verdicts") && argc > 2) return all(argv[2]);
  if (!strcmp(mode, "cuts") && argc > 2) return cuts(argv[2]);
  fprintf(stderr, "usage: result_walk_main verdicts FILE | cuts FILE\n");
  return 2;
}
