// Stand-alone host program over mapper_amd/csrc/xm_sam_rules.h (built and run by tests/test_sam_rules.py, with the address and undefined-behaviour
// sanitizers where the compiler has them; never loaded into Python): the rules the SAM kernels apply, run on the host.
//   doubles [FILE]   Double.toString of the rules against std::to_chars rearranged as xm_hostio.cpp's javaDouble does, over the corpus of the test plan (and the
//                    raw doubles of FILE); "ok <values> maxlen <n>" or "diff <bits> <got> <want>"
//   strings FILE     the rules' string of every raw double of FILE, one a line
//   format FILE      the SAM text of a case file (tests/sam_cases.py write_case): "ok <bytes> <records>\n" and the text, or "malformed <query>\n"
//   cut FILE         the one query of the case file with its int slice, then its double slice, cut short at every length, each in a heap block of exactly
//                    that size: every cut must be malformed (and the sanitizer sees any read behind the end); "cut ok <ints> <dbls>"
#include "../mapper_amd/csrc/xm_sam_rules.h"

#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

std::string wantDouble(double x) {  // xm_hostio.cpp javaDouble
  std::string out;
  if (x != x) return "NaN";
  if (x == 0) return "0.0";
  if (x > 1.7976931348623157e308) return "Infinity";
  if (x < -1.7976931348623157e308) return "-Infinity";
  char buf[64];
  auto res = std::to_chars(buf, buf + sizeof(buf), x, std::chars_format::scientific);
  std::string s(buf, res.ptr);
  size_t i = 0;
  bool neg = false;
  if (s[0] == '-') { neg = true; i = 1; }
  const size_t e = s.find('e');
  std::string digits;
  for (size_t k = i; k < e; k++) if (s[k] != '.') digits += s[k];
  const int exp10 = atoi(s.c_str() + e + 1);
  const double a = x < 0 ? -x : x;
  if (neg) out += '-';
  if (a >= 1e-3 && a < 1e7) {
    if (exp10 >= 0) {
      const size_t intDigits = (size_t)exp10 + 1;
      if (digits.size() <= intDigits) { out += digits; out.append(intDigits - digits.size(), '0'); out += ".0"; }
      else { out.append(digits, 0, intDigits); out += '.'; out.append(digits, intDigits, std::string::npos); }
    } else {
      out += "0.";
      out.append((size_t)(-exp10 - 1), '0');
      out += digits;
    }
  } else {
    out += digits[0];
    out += '.';
    if (digits.size() > 1) out.append(digits, 1, std::string::npos); else out += '0';
    out += 'E';
    out += std::to_string(exp10);
  }
  return out;
}

long long g_values = 0;
int g_maxLen = 0;

bool checkDouble(double x) {
  char* got = new char[xm::XM_SAM_DOUBLE_BYTES];  // (a heap block of exactly the promised size: the sanitizer sees a longer string)
  const int n = xm::samPutDouble(got, x);
  const std::string want = wantDouble(x);
  const bool ok = n <= xm::XM_SAM_DOUBLE_BYTES && want == std::string(got, (size_t)n);
  if (!ok) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    printf("diff %016llx %.*s %s\n", (unsigned long long)bits, n, got, want.c_str());
  }
  delete[] got;
  g_values++;
  if (n > g_maxLen) g_maxLen = n;
  return ok;
}

bool checkWithNeighbours(double x) {
  return checkDouble(x) && checkDouble(std::nextafter(x, std::numeric_limits<double>::infinity())) && checkDouble(std::nextafter(x, -std::numeric_limits<double>::infinity())) &&
         checkDouble(-x);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t nextRandom() {  // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return g_rng * 0x2545F4914F6CDD1Dull;
}

std::vector<char> readFile(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  std::vector<char> data;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  return data;
}

int doubles(const char* file) {
  // the two logarithm shortcuts against the table's exact exponents: floor(log10 2^e) = k <=> 10^k <= 2^e < 10^(k+1), and floor(log2 10^k) = e2[k]
  const xm::SamPow10Table& t = xm::samPow10();
  auto e2 = [&](int k) { return t.e2[k - xm::XM_SAM_POW10_MIN]; };
  for (int e = -960; e <= 1070; e++) {  // (where k and k + 1 are powers the table holds)
    const int k = xm::samFloorLog10Pow2(e);
    // 10^k <= 2^e: e2(k) < e, or e2(k) == e and 10^k is a power of two (k == 0);  2^e < 10^(k+1): e2(k+1) >= e (10^(k+1) is no power of two unless k + 1 == 0, where it equals 2^0)
    const bool low = e2(k) < e || (k == 0 && e2(k) == e);
    const bool high = e2(k + 1) >= e && !(k + 1 == 0 && e >= 0);
    if (!low || !high) { printf("diff log10pow2 %d %d\n", e, k); return 1; }
    // 3/4 * 2^e = 3 * 2^(e-2): 10^k3 <= 3 * 2^(e-2) < 10^(k3+1), decided on the first 64 bits of 10^k (3 * 2^(e-2) has two)
    const int k3 = xm::samFloorLog10ThreeQuartersPow2(e);
    auto atMost = [&](int k10) {  // 10^k10 <= 3 * 2^(e-2)
      const int x = e2(k10);
      if (x != e - 1) return x < e - 1;  // (3 * 2^(e-2) lies in [2^(e-1), 2^e))
      const uint64_t hi = t.hi[k10 - xm::XM_SAM_POW10_MIN], lo = t.lo[k10 - xm::XM_SAM_POW10_MIN];
      return hi < (3ull << 62) || (hi == (3ull << 62) && lo == 0);
    };
    if (!atMost(k3) || atMost(k3 + 1)) { printf("diff log10threequarters %d %d\n", e, k3); return 1; }
  }
  if (file) {
    const std::vector<char> raw = readFile(file);
    for (size_t i = 0; i + 8 <= raw.size(); i += 8) { double x; memcpy(&x, raw.data() + i, 8); if (!checkDouble(x)) return 1; }
  }
  for (int e = -1074; e <= 1023; e++) if (!checkWithNeighbours(std::ldexp(1.0, e))) return 1;
  for (int k = -323; k <= 308; k++) {
    char text[16];
    snprintf(text, sizeof(text), "1e%d", k);
    if (!checkWithNeighbours(strtod(text, nullptr))) return 1;
  }
  const double edges[] = {5e-324, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308, 9999999.999999998, 1.0E7, 0.001, 9.999999999999999E-4, -0.0, 0.0,
                          std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  for (double x : edges) if (!checkDouble(x) || !checkDouble(-x)) return 1;
  for (int i = 0; i < 1200000; i++) {
    const uint64_t bits = nextRandom();
    double x;
    memcpy(&x, &bits, 8);
    if (!checkDouble(x)) return 1;
  }
  // penalties as the aligner adds them up: a * 1 + b * 1.5 + c * 0.5 + d * 0.6 + e * 0.1, in that order
  long long sums = 0;
  for (int a = 0; a < 12; a++) for (int b = 0; b < 12; b++) for (int c = 0; c < 12; c++) for (int d = 0; d < 26; d++) for (int e = 0; e < 26; e++) {
    double x = 0;
    for (int i = 0; i < a; i++) x += 1.0;
    for (int i = 0; i < b; i++) x += 1.5;
    for (int i = 0; i < c; i++) x += 0.5;
    for (int i = 0; i < d; i++) x += 0.6;
    for (int i = 0; i < e; i++) x += 0.1;
    if (!checkDouble(x)) return 1;
    sums++;
  }
  if (sums < 1000000 || g_maxLen > xm::XM_SAM_DOUBLE_BYTES) { printf("diff corpus %lld %d\n", sums, g_maxLen); return 1; }
  printf("ok %lld maxlen %d\n", g_values, g_maxLen);
  return 0;
}

// a case file: eight int64 (nq, codes, name bytes, ints, dbls, contigs, contig name bytes, 0), then the arrays in the order of Case's members
struct Case {
  int64_t head[8];
  std::vector<int32_t> mateCount;
  std::vector<int64_t> mateOffset;
  std::vector<int32_t> mateLength;
  std::vector<uint8_t> codes;
  std::vector<char> names;
  std::vector<int64_t> nameOff;
  std::vector<int32_t> ints;
  std::vector<double> dbls;
  std::vector<int64_t> intOff, dblOff;
  std::vector<char> contigNames;
  std::vector<int64_t> contigOff;
  const char* at = nullptr;
  const char* end = nullptr;
  template <class T> void take(std::vector<T>& v, int64_t n) {
    if (n < 0 || (int64_t)(end - at) < n * (int64_t)sizeof(T)) { fprintf(stderr, "case file too short\n"); exit(2); }
    v.resize((size_t)n);
    if (n) memcpy(v.data(), at, (size_t)n * sizeof(T));
    at += (size_t)n * sizeof(T);
  }
  explicit Case(const char* path) {
    const std::vector<char> raw = readFile(path);
    at = raw.data(); end = raw.data() + raw.size();
    std::vector<int64_t> h;
    take(h, 8);
    memcpy(head, h.data(), sizeof(head));
    const int64_t nq = head[0];
    take(mateCount, nq); take(mateOffset, 2 * nq); take(mateLength, 2 * nq); take(codes, head[1]); take(names, head[2]); take(nameOff, 2 * nq + 1);
    take(ints, head[3]); take(dbls, head[4]); take(intOff, nq + 1); take(dblOff, nq + 1); take(contigNames, head[6]); take(contigOff, head[5] + 1);
    at = end = nullptr;
  }
  xm::SamBatch batch() const { return xm::SamBatch{head[0], mateCount.data(), mateOffset.data(), mateLength.data(), codes.data(), names.data(), nameOff.data()}; }
  xm::SamContigs contigs() const { return xm::SamContigs{(int32_t)head[5], contigNames.data(), contigOff.data()}; }
};

struct StringSink {
  std::string text;
  long long records = 0;
  template <class F> void compose(F f) {
    char* room = new char[xm::XM_SAM_ROOM];  // (exactly the promised room, on the heap)
    const int n = f(room);
    if (n > xm::XM_SAM_ROOM) { fprintf(stderr, "a compose wrote %d bytes\n", n); exit(3); }
    text.append(room, (size_t)n);
    delete[] room;
  }
  void bytesAt(const char* p, long long n) { text.append(p, (size_t)n); }
  void seq(const uint8_t* codes, int n, bool rev) { for (int i = 0; i < n; i++) text += xm::samSeqBase(codes, n, rev, i); }
  void endRecord() { records++; }
};

int format(const char* path) {
  const Case c(path);
  const xm::SamBatch b = c.batch();
  const xm::SamContigs contigs = c.contigs();
  const xm::SamStreams st{c.ints.data(), c.dbls.data(), c.intOff.data(), c.dblOff.data()};
  StringSink all;
  for (int64_t q = 0; q < b.nq; q++) {
    xm::SamCount count;
    if (!xm::samWalkQuery(b, st, contigs, q, count)) { printf("malformed %lld\n", (long long)q); return 0; }
    const size_t before = all.text.size();
    const long long recordsBefore = all.records;
    if (!xm::samWalkQuery(b, st, contigs, q, all)) { printf("malformed %lld\n", (long long)q); return 0; }
    if ((long long)(all.text.size() - before) != count.bytes || all.records - recordsBefore != count.records) {
      fprintf(stderr, "query %lld: measured %lld bytes, %lld records; wrote %zu, %lld\n", (long long)q, count.bytes, count.records, all.text.size() - before, all.records - recordsBefore);
      return 3;
    }
  }
  printf("ok %zu %lld\n", all.text.size(), all.records);
  fwrite(all.text.data(), 1, all.text.size(), stdout);
  return 0;
}

int cut(const char* path) {
  const Case c(path);
  if (c.head[0] != 1) { fprintf(stderr, "cut takes a case of one query\n"); return 2; }
  const xm::SamBatch b = c.batch();
  const xm::SamContigs contigs = c.contigs();
  const int64_t ni = (int64_t)c.ints.size(), nd = (int64_t)c.dbls.size();
  for (int64_t len = 0; len <= ni; len++) {
    int32_t* ints = new int32_t[(size_t)len];
    if (len) memcpy(ints, c.ints.data(), sizeof(int32_t) * (size_t)len);
    const int64_t intOff[2] = {0, len};
    const xm::SamStreams st{ints, c.dbls.data(), intOff, c.dblOff.data()};
    xm::SamCount count;
    const bool ok = xm::samWalkQuery(b, st, contigs, 0, count);
    delete[] ints;
    if (ok != (len == ni)) { printf("cut ints %lld of %lld: %s\n", (long long)len, (long long)ni, ok ? "accepted" : "malformed"); return 0; }
  }
  for (int64_t len = 0; len < nd; len++) {
    double* dbls = new double[(size_t)len];
    if (len) memcpy(dbls, c.dbls.data(), sizeof(double) * (size_t)len);
    const int64_t dblOff[2] = {0, len};
    const xm::SamStreams st{c.ints.data(), dbls, c.intOff.data(), dblOff};
    xm::SamCount count;
    const bool ok = xm::samWalkQuery(b, st, contigs, 0, count);
    delete[] dbls;
    if (ok) { printf("cut dbls %lld of %lld: accepted\n", (long long)len, (long long)nd); return 0; }
  }
  printf("cut ok %lld %lld\n", (long long)ni, (long long)nd);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "doubles") return doubles(argc > 2 ? argv[2] : nullptr);
  if (mode == "strings" && argc > 2) {
    const std::vector<char> raw = readFile(argv[2]);
    for (size_t i = 0; i + 8 <= raw.size(); i += 8) {
      double x;
      memcpy(&x, raw.data() + i, 8);
      char out[xm::XM_SAM_DOUBLE_BYTES];
      const int n = xm::samPutDouble(out, x);
      printf("%.*s\n", n, out);
    }
    return 0;
  }
  if (mode == "format" && argc > 2) return format(argv[2]);
  if (mode == "cut" && argc > 2) return cut(argv[2]);
  fprintf(stderr, "usage: sam_rules_main doubles [FILE] | strings FILE | format FILE | cut FILE\n");
  return 2;
}
