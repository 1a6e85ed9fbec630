// The rules of the count per combination of contigs (mapper_amd/csrc/xm_refs_rules.h: plain C++ that the kernels of xm_refs.h call) run on the host, for
// tests/test_refs_rules.py, which builds this file with g++ (with -fsanitize=address,undefined where the host compiler has the runtime).
//   refs_rules_main count FILE BITS   the four stages of xm_refs.h restated for one thread - claim, verify and tally, offsets, gather - over every query of the
//                                     case, with fingerprints of BITS bits: "ok nq aligned records leftover", then a line per record "count n id ...", then a
//                                     line per left-over query with the contigs of its sequence alignments; or "malformed Q" with the lowest malformed query
//   refs_rules_main cut FILE          a case of one query: its slice cut short at every position, each cut in a heap block of its own size (a read behind
//                                     the cut is a read behind the block: the sanitizer build stops there), must be malformed
//   refs_rules_main fingerprints      refsFingerprint over many sets and every width: never 0, nothing above the width, and refsInsert against a sort
// FILE: int64 head[4] = queries, ints, doubles, contigs; then ints, dbls, int_off[nq + 1], dbl_off[nq + 1] (tests/summary_cases.py write_streams).
#include "../mapper_amd/csrc/xm_refs_rules.h"

#include <algorithm>
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

// the gather's sink: the contig of sequence alignment k at out[lo + k], inside [lo, hi) only
struct ContigStore {
  std::vector<int32_t>& out;
  long long lo, hi;
  void contig(long long k, int32_t c) {
    if (k >= 0 && lo + k < hi && lo + k < (long long)out.size()) out[(size_t)(lo + k)] = c;
  }
};

int count(const char* path, int bits) {
  const Case c(path);
  const xm::SummaryStreams st = c.streams();
  const long long nq = c.head[0];
  size_t cap = 2;
  while (cap < 2 * (size_t)nq) cap <<= 1;
  const unsigned long long mask = cap - 1, none = ~0ull;
  std::vector<unsigned long long> keys(cap, 0), reps(cap, none), counts(cap, 0);
  std::vector<int32_t> slotOf((size_t)nq), leftLen((size_t)nq), leftFlag((size_t)nq), isRep((size_t)nq);
  unsigned long long malformed = none, aligned = 0;
  // claim
  for (long long q = 0; q < nq; q++) {
    xm::RefSet s;
    if (!xm::refsWalkQuery(st, q, s)) { malformed = std::min(malformed, (unsigned long long)q); s = xm::RefSet(); }
    aligned += s.aligned ? 1 : 0;
    int32_t slot = -1;
    if (s.aligned && s.wide) slot = -2;
    if (s.aligned && !s.wide) {
      const unsigned long long h = xm::refsFingerprint(s.ids, s.n, bits);
      unsigned long long at = h & mask;
      while (keys[at] != 0 && keys[at] != h) at = (at + 1) & mask;
      keys[at] = h;
      reps[at] = std::min(reps[at], (unsigned long long)q);
      slot = (int32_t)at;
    }
    slotOf[(size_t)q] = slot;
    leftLen[(size_t)q] = slot == -2 ? s.nSeq : 0;
    leftFlag[(size_t)q] = slot == -2 ? 1 : 0;
  }
  // verify and tally
  for (long long q = 0; q < nq; q++) {
    const int32_t slot = slotOf[(size_t)q];
    bool rep = false;
    if (slot >= 0) {
      const unsigned long long r = reps[(size_t)slot];
      rep = r == (unsigned long long)q;
      bool counted = rep;
      if (!rep) {
        xm::RefSet mine, theirs;
        const bool ok = r < (unsigned long long)nq && xm::refsWalkQuery(st, q, mine) && xm::refsWalkQuery(st, (long long)r, theirs);
        counted = ok && mine.aligned && theirs.aligned && xm::refsSame(mine, theirs);
        if (!counted) { slotOf[(size_t)q] = -2; leftLen[(size_t)q] = ok ? mine.nSeq : 0; leftFlag[(size_t)q] = ok ? 1 : 0; }
      }
      if (counted) counts[(size_t)slot]++;
    }
    isRep[(size_t)q] = rep ? 1 : 0;
  }
  if (malformed != none) { printf("malformed %llu\n", malformed); return 0; }
  // offsets
  std::vector<long long> off((size_t)nq + 1, 0), loff((size_t)nq + 1, 0), lqoff((size_t)nq + 1, 0);
  for (long long q = 0; q < nq; q++) {
    off[(size_t)q + 1] = off[(size_t)q] + isRep[(size_t)q];
    loff[(size_t)q + 1] = loff[(size_t)q] + leftLen[(size_t)q];
    lqoff[(size_t)q + 1] = lqoff[(size_t)q] + leftFlag[(size_t)q];
  }
  // gather
  struct Record { long long count; xm::RefSet set; };
  std::vector<Record> records((size_t)off[(size_t)nq]);
  std::vector<int32_t> left((size_t)loff[(size_t)nq], -1);
  std::vector<long long> leftStart((size_t)lqoff[(size_t)nq] + 1, -1);
  leftStart.back() = loff[(size_t)nq];
  for (long long q = 0; q < nq; q++) {
    if (off[(size_t)q + 1] > off[(size_t)q] && slotOf[(size_t)q] >= 0) {
      xm::RefSet s;
      if (xm::refsWalkQuery(st, q, s) && !s.wide) records[(size_t)off[(size_t)q]] = Record{(long long)counts[(size_t)slotOf[(size_t)q]], s};
    }
    if (loff[(size_t)q + 1] > loff[(size_t)q]) {
      ContigStore sink{left, loff[(size_t)q], loff[(size_t)q + 1]};
      xm::RefSet s;
      (void)xm::refsWalkQuery(st, q, s, sink);
    }
    if (lqoff[(size_t)q + 1] > lqoff[(size_t)q]) leftStart[(size_t)lqoff[(size_t)q]] = loff[(size_t)q];
  }
  printf("ok %lld %llu %zu %zu\n", nq, aligned, records.size(), leftStart.size() - 1);
  for (const Record& r : records) {
    printf("%lld %d", r.count, (int)r.set.n);
    for (int i = 0; i < r.set.n; i++) printf(" %d", (int)r.set.ids[i]);
    printf("\n");
  }
  for (size_t k = 0; k + 1 < leftStart.size(); k++) {
    for (long long i = leftStart[k]; i < leftStart[k + 1]; i++) printf("%d ", (int)left[(size_t)i]);
    printf("\n");
  }
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
    xm::RefSet s;
    const bool ok = xm::refsWalkQuery(st, 0, s);
    delete[] ints;
    if (ok != (len == ni)) { printf("cut ints %lld of %lld: %s\n", (long long)len, (long long)ni, ok ? "accepted" : "malformed"); return 0; }
  }
  for (int64_t len = 0; len < nd; len++) {  // (no double is read: only the slice's length counts, and nothing of the block of `len` doubles is touched)
    double* dbls = new double[(size_t)len];
    const int64_t dblOff[2] = {0, len};
    const xm::SummaryStreams st{c.ints.data(), dbls, c.intOff.data(), dblOff, (int32_t)c.head[3]};
    xm::RefSet s;
    const bool ok = xm::refsWalkQuery(st, 0, s);
    delete[] dbls;
    if (ok) { printf("cut dbls %lld of %lld: accepted\n", (long long)len, (long long)nd); return 0; }
  }
  printf("cut ok %lld %lld\n", (long long)ni, (long long)nd);
  return 0;
}

int fingerprints() {
  unsigned long long x = 88172645463325252ull;
  auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  long long sets = 0, wide = 0;
  for (int round = 0; round < 20000; round++) {
    const int draws = 1 + (int)(next() % 12), range = 1 + (int)(next() % 40);
    std::vector<int32_t> seen;
    xm::RefSet s;
    for (int k = 0; k < draws; k++) {
      const int32_t c = (int32_t)(next() % (unsigned)range);
      seen.push_back(c);
      xm::refsInsert(s, c);
    }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    if (s.wide != (seen.size() > (size_t)xm::XM_REFS_INLINE)) { printf("set %d: wide %d for %zu contigs\n", round, (int)s.wide, seen.size()); return 0; }
    if (s.wide) { wide++; continue; }
    if ((size_t)s.n != seen.size() || !std::equal(seen.begin(), seen.end(), s.ids)) { printf("set %d: not the sorted distinct contigs\n", round); return 0; }
    xm::RefSet same = s, other = s;
    other.ids[s.n - 1]++;
    if (!xm::refsSame(s, same) || xm::refsSame(s, other)) { printf("set %d: refsSame\n", round); return 0; }
    const unsigned long long whole = xm::refsFingerprint(s.ids, s.n, 64);
    for (int bits = 1; bits <= 64; bits++) {
      const unsigned long long h = xm::refsFingerprint(s.ids, s.n, bits);
      const unsigned long long cutTo = bits < 64 ? whole & ((1ull << bits) - 1) : whole;
      if (h == 0 || (bits < 64 && h >> bits) || h != (cutTo ? cutTo : 1)) { printf("set %d: fingerprint of %d bits\n", round, bits); return 0; }
    }
    sets++;
  }
  printf("fingerprints ok %lld %lld\n", sets, wide);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "count") && argc > 3) return count(argv[2], atoi(argv[3]));
  if (!strcmp(mode, "cut") && argc > 2) return cut(argv[2]);
  if (!strcmp(mode, "fingerprints")) return fingerprints();
  fprintf(stderr, "usage: refs_rules_main count FILE BITS | cut FILE | fingerprints\n");
  return 2;
}
