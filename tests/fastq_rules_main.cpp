// Stand-alone driver of mapper_amd/csrc/xm_fastq_rules.h for tests/test_fastq_text.py: the rules the FASTQ kernels (xm_fastq.h) apply on the device, applied
// here on the host, record by record, to one file or to a pair of files.  Usage: fastq_rules_main <file1> [<file2>].  Prints the batch arrays as the host
// reader (xmio_next with keep_qualities) gives them, one per line - numbers in decimal, bytes in hex:
//   nq <n> | mate_count .. | mate_offset .. | mate_length .. | codes <hex> | names <hex> | name_off .. | quals <hex> | qual_off .. | has_qual ..
// or, for a text that is not of the strict form, one line: error <file> <record> <FastqError>.
#include "../mapper_amd/csrc/xm_fastq_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace xm;

struct Text {
  std::string bytes;
  std::vector<long long> lineEnd;  // position of every '\n'; a last line without one ends at the size
};

static bool load(const char* path, Text& t) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) t.bytes.append(buf, n);
  fclose(f);
  const char* p = t.bytes.data();
  const long long size = (long long)t.bytes.size();
  long long at = 0;
  while (at < size) {
    const char* nl = (const char*)memchr(p + at, '\n', (size_t)(size - at));
    if (!nl) { t.lineEnd.push_back(size); break; }
    t.lineEnd.push_back(nl - p);
    at = (nl - p) + 1;
  }
  return true;
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

int main(int argc, char** argv) {
  if (argc < 2 || argc > 3) { fprintf(stderr, "usage: fastq_rules_main <file1> [<file2>]\n"); return 2; }
  const bool paired = argc == 3;
  Text texts[2];
  for (int k = 0; k < (paired ? 2 : 1); k++)
    if (!load(argv[1 + k], texts[k])) { fprintf(stderr, "cannot read %s\n", argv[1 + k]); return 2; }
  for (int k = 0; k < (paired ? 2 : 1); k++)
    if (texts[k].lineEnd.size() % 4 != 0) { printf("error %d %lld %d\n", k, (long long)(texts[k].lineEnd.size() / 4), (int)XM_FQ_LINE_COUNT); return 0; }
  const long long nq = (long long)texts[0].lineEnd.size() / 4;
  if (paired && (long long)texts[1].lineEnd.size() / 4 != nq) { printf("error 1 %lld %d\n", nq, (int)XM_FQ_LINE_COUNT); return 0; }
  // the fields of every mate slot in batch order, strict-form errors first (the lowest (file, record) is the one reported)
  std::vector<FastqFields> fields((size_t)(2 * nq));
  for (int file = 0; file < (paired ? 2 : 1); file++) {
    const Text& t = texts[file];
    for (long long r = 0; r < nq; r++) {
      const long long l = 4 * r;
      const long long s0 = l == 0 ? 0 : t.lineEnd[(size_t)l - 1] + 1;
      FastqFields f;
      const int err = fastqRecord(t.bytes.data(), s0, t.lineEnd[(size_t)l], t.lineEnd[(size_t)l] + 1, t.lineEnd[(size_t)l + 1], t.lineEnd[(size_t)l + 2] + 1, t.lineEnd[(size_t)l + 3], f);
      if (err != XM_FQ_OK) { printf("error %d %lld %d\n", file, r, err); return 0; }
      fields[(size_t)fastqMateSlot(r, file)] = f;
    }
  }
  std::vector<int> mateCount, mateLength, hasQual;
  std::vector<long long> mateOffset, nameOff, qualOff;
  std::string codes, names, quals;
  for (long long slot = 0; slot < 2 * nq; slot++) {
    if ((slot & 1) == 0) mateCount.push_back(paired ? 2 : 1);
    nameOff.push_back((long long)names.size());
    qualOff.push_back((long long)quals.size());
    if (fastqPaddingMate(slot, paired)) { mateOffset.push_back(0); mateLength.push_back(0); hasQual.push_back(0); continue; }
    const FastqFields& f = fields[(size_t)slot];
    const std::string& text = texts[paired ? (slot & 1) : 0].bytes;
    mateOffset.push_back((long long)codes.size());
    mateLength.push_back((int)f.seqLen);
    hasQual.push_back(1);
    for (long long i = 0; i < f.seqLen; i++) codes.push_back((char)fastqCode((unsigned char)text[(size_t)(f.seqAt + i)]));
    names.append(text, (size_t)f.nameAt, (size_t)f.nameLen);
    quals.append(text, (size_t)f.qualAt, (size_t)f.qualLen);
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
