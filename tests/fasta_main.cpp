// Stand-alone driver of mapper_amd/csrc/xm_fasta_rules.h for tests/test_fasta_text.py: what the kernels of xm_fasta.h do (the line ends, the lines, the two
// scans over them, the records, with a split size their sections, the offsets, the gather by base ordinal), restated for one thread on the host over the
// very rule functions the kernels call.
//   fasta_main stage <split> <file1> [<file2>]                                         the counts announced are the ones the texts hold
//   fasta_main stage <split> <file1> <file2 or -> <records1> <lines1> [<records2> <lines2>]   other counts announced
// -> the batch arrays as tests/fastq_split_main.cpp prints them, or "error <file> <record> <FastaError>"
#include "../mapper_amd/csrc/xm_fasta_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace xm;

struct Text {
  std::string text;
  long long records = 0, lines = 0;  // announced
  std::vector<long long> lineEnd, lineStart, lineBases, baseBefore, recLine;
  std::vector<int> lineHeader;
  long long headers = 0;
};

static bool readFile(const char* path, std::string& text) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); return false; }
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
  fclose(f);
  return true;
}

// stages 1 to 3: the line ends (a last line without '\n' ends at the size), what every line is, the scans of the header flags and of the trimmed lengths
static void lines(Text& t) {
  const long long size = (long long)t.text.size();
  for (long long at = 0; at < size;) {
    const char* nl = (const char*)memchr(t.text.data() + at, '\n', (size_t)(size - at));
    if (!nl) { t.lineEnd.push_back(size); break; }
    t.lineEnd.push_back(nl - t.text.data());
    at = (nl - t.text.data()) + 1;
  }
  const size_t n = t.lineEnd.size();
  long long bases = 0;
  for (size_t i = 0; i < n; i++) {
    const long long start = i == 0 ? 0 : t.lineEnd[i - 1] + 1;
    long long at, length;
    const bool header = fastaLine(t.text.data(), start, t.lineEnd[i], at, length);
    t.lineStart.push_back(header ? start : at);
    t.lineBases.push_back(header ? 0 : length);
    t.lineHeader.push_back(header ? 1 : 0);
    t.baseBefore.push_back(bases);
    if (header) t.recLine.push_back((long long)i);
    bases += t.lineBases.back();
  }
  t.baseBefore.push_back(bases);
  t.headers = (long long)t.recLine.size();
  t.recLine.push_back((long long)n);
}

// stage 4: record r -> its name and its ordinals
static FastqFields recordOf(const Text& t, long long r) {
  FastqFields f;
  const long long line = t.recLine[(size_t)r], next = t.recLine[(size_t)r + 1];
  long long at, length;
  fastaLine(t.text.data(), t.lineStart[(size_t)line], t.lineEnd[(size_t)line], at, length);
  f.nameAt = at; f.nameLen = length;
  f.seqAt = t.baseBefore[(size_t)line];
  f.seqLen = t.baseBefore[(size_t)next] - f.seqAt;
  f.qualAt = 0; f.qualLen = 0;
  return f;
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

struct Mate { FastqFields f; int file; };

static int stage(int argc, char** argv) {
  const long long split = atoll(argv[2]);
  Text t[2];
  const bool paired = argc > 4 && strcmp(argv[4], "-") != 0;
  if (!readFile(argv[3], t[0].text) || (paired && !readFile(argv[4], t[1].text))) return 2;
  if (split > 0 && paired) { fprintf(stderr, "pairs are not cut into sections\n"); return 2; }
  const int files = paired ? 2 : 1;
  unsigned long long firstError = ~0ull;  // (file << 48) | (record << 8) | FastaError: the lowest wins
  auto refuse = [&](int file, long long record, int err) {
    const unsigned long long key = ((unsigned long long)file << 48) | ((unsigned long long)record << 8) | (unsigned long long)err;
    if (key < firstError) firstError = key;
  };
  for (int k = 0; k < files; k++) {
    if (t[k].text.empty()) { fprintf(stderr, "an empty text\n"); return 2; }
    lines(t[k]);
    t[k].records = t[k].headers;
    t[k].lines = (long long)t[k].lineEnd.size();
    if (argc > 5 + 2 * k + 1) { t[k].records = atoll(argv[5 + 2 * k]); t[k].lines = atoll(argv[6 + 2 * k]); }
    if (t[k].text[0] != '>') refuse(k, 0, XM_FA_NO_HEADER);
  }
  bool countsHold = true;
  for (int k = 0; k < files; k++) countsHold = countsHold && t[k].lines == (long long)t[k].lineEnd.size() && t[k].records == t[k].headers;
  if (paired && t[0].records != t[1].records) { fprintf(stderr, "paired texts of different numbers of records\n"); return 2; }
  // stage 4 (and with a split size 2a-2c): the mate slots
  std::vector<Mate> mates;
  std::vector<int> mateCount;
  FastqFields pad;
  pad.nameAt = pad.seqAt = pad.qualAt = 0;
  pad.nameLen = pad.seqLen = pad.qualLen = 0;
  if (countsHold) {
    const long long records = t[0].records;
    if (split == 0) {
      for (long long r = 0; r < records; r++) {
        for (int k = 0; k < 2; k++) {
          if (k == 1 && !paired) { mates.push_back(Mate{pad, 0}); continue; }
          const FastqFields f = recordOf(t[k], r);
          const int err = fastaRecordError(f.seqLen, 0);
          if (err != XM_FA_OK) refuse(k, r, err);
          mates.push_back(Mate{f, k});
        }
        mateCount.push_back(paired ? 2 : 1);
      }
    } else {
      std::vector<FastqFields> recs;
      std::vector<long long> first;
      long long nq = 0;
      for (long long r = 0; r < records; r++) {
        recs.push_back(recordOf(t[0], r));
        const int err = fastaRecordError(recs.back().seqLen, split);
        if (err != XM_FA_OK) refuse(0, r, err);
        first.push_back(nq);
        nq += err == XM_FA_OK ? fastqSectionCount(recs.back().seqLen, split) : 0;
      }
      first.push_back(nq);
      for (long long q = 0; q < nq && firstError == ~0ull; q++) {
        long long lo = 0, hi = records;
        while (hi - lo > 1) {
          const long long mid = (lo + hi) >> 1;
          if (first[(size_t)mid] <= q) lo = mid; else hi = mid;
        }
        FastqFields m;
        fastqSectionMate(recs[(size_t)lo], first[(size_t)lo + 1] - first[(size_t)lo], q - first[(size_t)lo], m);
        mates.push_back(Mate{m, 0});
        mates.push_back(Mate{pad, 0});
        mateCount.push_back(1);
      }
    }
  }
  if (firstError != ~0ull) {
    printf("error %d %lld %d\n", (int)(firstError >> 48), (long long)((firstError >> 8) & 0xFFFFFFFFFFull), (int)(firstError & 0xFF));
    return 0;
  }
  for (int k = 0; k < files; k++) {
    const long long record = t[k].headers < t[k].records ? t[k].headers : t[k].records;
    if (t[k].lines != (long long)t[k].lineEnd.size()) { printf("error %d %lld %d\n", k, record, (int)XM_FA_LINE_COUNT); return 0; }
    if (t[k].records != t[k].headers) { printf("error %d %lld %d\n", k, record, (int)XM_FA_RECORD_COUNT); return 0; }
  }
  // stages 5 and 6: the offsets of the slots, then the gather - every base by its ordinal, through fastaLineOf and the line's start
  std::vector<long long> mateOffset, mateLength, nameOff, qualOff;
  std::vector<int> hasQual;
  std::string codes, names, quals;
  for (const Mate& m : mates) {
    const Text& x = t[m.file];
    mateOffset.push_back(m.f.seqLen > 0 ? (long long)codes.size() : 0);
    mateLength.push_back(m.f.seqLen);
    nameOff.push_back((long long)names.size());
    qualOff.push_back(0);
    hasQual.push_back(0);
    for (long long b = m.f.seqAt; b < m.f.seqAt + m.f.seqLen; b++) {
      const long long line = fastaLineOf(x.baseBefore.data(), (long long)x.lineEnd.size(), b);
      const long long src = x.lineStart[(size_t)line] + (b - x.baseBefore[(size_t)line]);
      codes.push_back((char)fastqCode((unsigned char)x.text[(size_t)src]));
    }
    names.append(x.text, (size_t)m.f.nameAt, (size_t)m.f.nameLen);
  }
  nameOff.push_back((long long)names.size());
  qualOff.push_back(0);
  printf("nq %lld\n", (long long)mateCount.size());
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
  if (argc >= 4 && !strcmp(argv[1], "stage")) return stage(argc, argv);
  fprintf(stderr, "usage: fasta_main stage <split> <file1> [<file2 or -> [<records1> <lines1> [<records2> <lines2>]]]\n");
  return 2;
}
