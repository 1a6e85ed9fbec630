// Stand-alone driver of the split form of mapper_amd/csrc/xm_fastq_rules.h for tests/test_fastq_split.py: what the kernels of xm_fastq.h do with a split size
// (stages 2a, 2b, 2c, 3 and 4), restated for one thread on the host over the very rule functions the kernels call.
//   fastq_split_main rule <length> <split> [<k> ...]   every section of the rule is checked here (they partition [0, length), none is empty or longer than
//                                                      <split>; past 2^22 sections: the first and the last 2^20 and every 1021st between them) -> "count <n>",
//                                                      then one line "<k> <start> <end>" for every <k> given (none given: for every section)
//   fastq_split_main grid <lengths> <splits>           "<length> <split> <start> <end> <start> <end> ..." for every length 1 .. <lengths> and split 1 .. <splits>
//   fastq_split_main stage <file> <split>              the batch arrays as tests/fastq_rules_main.cpp prints them, or "error 0 <record> <FastqError>"
#include "../mapper_amd/csrc/xm_fastq_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace xm;

static int checkSection(long long length, long long split, long long count, long long k, long long& expectStart) {
  long long start, end;
  fastqSection(length, count, k, start, end);
  if (expectStart >= 0 && start != expectStart) { printf("gap %lld %lld %lld\n", k, start, expectStart); return 1; }
  if (end <= start || end - start > split || start < 0 || end > length) { printf("bad %lld %lld %lld\n", k, start, end); return 1; }
  expectStart = end;
  return 0;
}

static int rule(int argc, char** argv) {
  const long long length = atoll(argv[2]), split = atoll(argv[3]);
  const long long count = fastqSectionCount(length, split);
  long long start, end;
  fastqSection(length, count, 0, start, end);
  if (start != 0) { printf("bad first %lld\n", start); return 0; }
  fastqSection(length, count, count - 1, start, end);
  if (end != length) { printf("bad last %lld\n", end); return 0; }
  const long long window = 1ll << 20;
  long long expect = 0;
  if (count <= 4 * window) {
    for (long long k = 0; k < count; k++) if (checkSection(length, split, count, k, expect)) return 0;
  } else {
    for (long long k = 0; k < window; k++) if (checkSection(length, split, count, k, expect)) return 0;
    for (long long k = window; k < count - window; k += 1021) {  // (section k + 1 starts where section k ends: two neighbours each)
      expect = -1;
      if (checkSection(length, split, count, k, expect) || checkSection(length, split, count, k + 1, expect)) return 0;
    }
    expect = -1;
    for (long long k = count - window; k < count; k++) if (checkSection(length, split, count, k, expect)) return 0;
  }
  printf("count %lld\n", count);
  if (argc > 4) {
    for (int a = 4; a < argc; a++) {
      const long long k = atoll(argv[a]);
      fastqSection(length, count, k, start, end);
      printf("%lld %lld %lld\n", k, start, end);
    }
  } else {
    for (long long k = 0; k < count; k++) {
      fastqSection(length, count, k, start, end);
      printf("%lld %lld %lld\n", k, start, end);
    }
  }
  return 0;
}

static int grid(char** argv) {
  const long long lengths = atoll(argv[2]), splits = atoll(argv[3]);
  for (long long length = 1; length <= lengths; length++)
    for (long long split = 1; split <= splits; split++) {
      const long long count = fastqSectionCount(length, split);
      printf("%lld %lld", length, split);
      for (long long k = 0; k < count; k++) {
        long long start, end;
        fastqSection(length, count, k, start, end);
        printf(" %lld %lld", start, end);
      }
      printf("\n");
    }
  return 0;
}

template <class T>
static void printNumbers(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (const T& x : v) printf(" %lld", (long long)x);
  printf("\n");
}
static void printHex(const char* name, const std::string& s) {
  printf("%s ", name);
  for (unsigned char c : s) printf("%02x", c);
  printf("\n");
}

static int stage(char** argv) {
  const long long split = atoll(argv[3]);
  std::string text;
  FILE* f = fopen(argv[2], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
  fclose(f);
  // stage 1: the line ends (a last line without '\n' ends at the size)
  std::vector<long long> lineEnd;
  const long long size = (long long)text.size();
  for (long long at = 0; at < size;) {
    const char* nl = (const char*)memchr(text.data() + at, '\n', (size_t)(size - at));
    if (!nl) { lineEnd.push_back(size); break; }
    lineEnd.push_back(nl - text.data());
    at = (nl - text.data()) + 1;
  }
  if (lineEnd.size() % 4 != 0) { printf("error 0 %lld %d\n", (long long)(lineEnd.size() / 4), (int)XM_FQ_LINE_COUNT); return 0; }
  const long long records = (long long)lineEnd.size() / 4;
  // stage 2a: a record's fields and its section count (xm_fastq_split_records_kernel)
  std::vector<FastqFields> recs((size_t)records);
  std::vector<long long> counts((size_t)records);
  for (long long r = 0; r < records; r++) {
    const size_t l = (size_t)(4 * r);
    const long long s0 = l == 0 ? 0 : lineEnd[l - 1] + 1;
    const int err = fastqRecordSplit(text.data(), s0, lineEnd[l], lineEnd[l] + 1, lineEnd[l + 1], lineEnd[l + 2] + 1, lineEnd[l + 3], recs[(size_t)r]);
    if (err != XM_FQ_OK) { printf("error 0 %lld %d\n", r, err); return 0; }
    counts[(size_t)r] = fastqSectionCount(recs[(size_t)r].seqLen, split);
  }
  // stage 2b: the exclusive scan of the counts (xm_fastq_split_sums / blocks / first_kernel)
  std::vector<long long> first((size_t)records + 1);
  long long nq = 0;
  for (long long r = 0; r < records; r++) { first[(size_t)r] = nq; nq += counts[(size_t)r]; }
  first[(size_t)records] = nq;
  // stage 2c: a query finds its record by binary search and cuts its section (xm_fastq_split_sections_kernel)
  std::vector<FastqFields> mates((size_t)(2 * nq));
  std::vector<int> mateCount, mateLength((size_t)(2 * nq)), hasQual((size_t)(2 * nq));
  for (long long q = 0; q < nq; q++) {
    long long lo = 0, hi = records;
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (first[(size_t)mid] <= q) lo = mid; else hi = mid;
    }
    FastqFields m, pad;
    fastqSectionMate(recs[(size_t)lo], first[(size_t)lo + 1] - first[(size_t)lo], q - first[(size_t)lo], m);
    pad.nameAt = pad.seqAt = pad.qualAt = 0;
    pad.nameLen = pad.seqLen = pad.qualLen = 0;
    mates[(size_t)(2 * q)] = m;
    mates[(size_t)(2 * q + 1)] = pad;
    mateCount.push_back(1);
    mateLength[(size_t)(2 * q)] = (int)m.seqLen;
    mateLength[(size_t)(2 * q + 1)] = 0;
    hasQual[(size_t)(2 * q)] = hasQual[(size_t)(2 * q + 1)] = 0;
  }
  // stages 3 and 4, as without a split: the offsets of the slots, then bases -> codes and the name and quality bytes
  std::vector<long long> mateOffset, nameOff, qualOff;
  std::string codes, names, quals;
  for (long long slot = 0; slot < 2 * nq; slot++) {
    const FastqFields& m = mates[(size_t)slot];
    mateOffset.push_back(m.seqLen > 0 ? (long long)codes.size() : 0);
    nameOff.push_back((long long)names.size());
    qualOff.push_back((long long)quals.size());
    for (long long i = 0; i < m.seqLen; i++) codes.push_back((char)fastqCode((unsigned char)text[(size_t)(m.seqAt + i)]));
    names.append(text, (size_t)m.nameAt, (size_t)m.nameLen);
    quals.append(text, (size_t)m.qualAt, (size_t)m.qualLen);
  }
  nameOff.push_back((long long)names.size());
  qualOff.push_back((long long)quals.size());
  printf("nq %lld\n", nq);
  printNumbers("mate_count", mateCount);
  printNumbers("mate_offset", mateOffset);
  printNumbers("mate_length", mateLength);
  printHex("codes", codes);
  printHex("names", names);
  printNumbers("name_off", nameOff);
  printHex("quals", quals);
  printNumbers("qual_off", qualOff);
  printNumbers("has_qual", hasQual);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "rule")) return rule(argc, argv);
  if (argc == 4 && !strcmp(argv[1], "grid")) return grid(argv);
  if (argc == 4 && !strcmp(argv[1], "stage")) return stage(argv);
  fprintf(stderr, "usage: fastq_split_main rule <length> <split> [<k> ...] | grid <lengths> <splits> | stage <file> <split>\n");
  return 2;
}
