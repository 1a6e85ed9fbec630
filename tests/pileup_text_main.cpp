// Stand-alone host program over mapper_amd/csrc/xm_pileup_text_rules.h (built and run by tests/test_pileup_text_rules.py, with the address and
// undefined-behaviour sanitizers where the compiler has them; never loaded into Python): the rules the kernels of xm_pileup_text.h and xm_pileup_add_last
// apply, run on the host.  Arrays come as raw files (numpy tofile) and go out raw on stdout.
//   text MATE_OFF MATE_LEN CODES EVENTS QUERY_BASE   the three stages as the kernels run them - kept length per event, exclusive sums, then byte by byte, each
//                                                    byte finding its event by the binary search - with every mate in a heap block of exactly its size (the
//                                                    sanitizer sees a read outside of it); out: int64 off[n + 1], then the text
//   append EVENTS OFF TEXT SPLIT                     pileupAppendCall over events [0, SPLIT) and then over [SPLIT, n) into one pile-up; out: int64 events[8 n],
//                                                    int64 off[n + 1], the text
//   page OFF FIRST N CAP                             pileupTextPage over the offsets; out: the number it returns, as text
#include "../mapper_amd/csrc/xm_pileup_text_rules.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

template <typename T>
std::vector<T> readAll(const char* path) {
  std::vector<T> out;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)bytes / sizeof(T));
  if (bytes && fread(out.data(), sizeof(T), out.size(), f) != out.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return out;
}

template <typename T>
void writeAll(const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), stdout) != v.size()) exit(2);
}

int text(char** a) {
  const std::vector<int64_t> mateOff = readAll<int64_t>(a[0]);
  const std::vector<int32_t> mateLen = readAll<int32_t>(a[1]);
  const std::vector<uint8_t> codes = readAll<uint8_t>(a[2]);
  const std::vector<long long> events = readAll<long long>(a[3]);
  const long long queryBase = atoll(a[4]);
  const long long nq = (long long)mateLen.size() / 2, n = (long long)events.size() / xm::XM_PILEUP_EVENT_WORDS;
  // every mate in a block of its own, of exactly its size
  std::vector<std::vector<uint8_t>> mates((size_t)nq * 2);
  for (size_t k = 0; k < mates.size(); k++) mates[k].assign(codes.begin() + mateOff[k], codes.begin() + mateOff[k] + mateLen[k]);
  auto mateOf = [&](const long long* ev, int& readLen) -> const uint8_t* {  // ptextMate of xm_pileup_text.h
    const long long q = ev[4] - queryBase;
    readLen = 0;
    if (q < 0 || q >= nq) return nullptr;
    const size_t k = (size_t)q * 2 + (size_t)xm::pileupEventMate(ev[5]);
    readLen = mateLen[k];
    return mates[k].data();
  };
  std::vector<int64_t> off((size_t)n + 1, 0);
  for (long long e = 0; e < n; e++) {  // measure, offsets
    const long long* ev = events.data() + e * xm::XM_PILEUP_EVENT_WORDS;
    int readLen;
    mateOf(ev, readLen);
    off[(size_t)e + 1] = off[(size_t)e] + xm::pileupTextKept(ev[2], ev[3], ev[6], readLen);
  }
  std::vector<char> out((size_t)off[(size_t)n]);
  for (long long b = 0; b < off[(size_t)n]; b++) {  // gather
    long long lo = 0, hi = n;
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (off[(size_t)mid] <= b) lo = mid; else hi = mid;
    }
    const long long* ev = events.data() + lo * xm::XM_PILEUP_EVENT_WORDS;
    int readLen;
    const uint8_t* mate = mateOf(ev, readLen);
    const long long i = b - off[(size_t)lo];
    if (i < 0 || b >= off[(size_t)lo + 1] || i >= xm::pileupTextKept(ev[2], ev[3], ev[6], readLen)) { fprintf(stderr, "byte %lld has no event\n", b); return 1; }
    out[(size_t)b] = xm::pileupTextByte(mate, readLen, xm::pileupEventReversed(ev[5]), ev[6], i);
  }
  writeAll(off);
  writeAll(out);
  return 0;
}

int append(char** a) {
  const std::vector<long long> events = readAll<long long>(a[0]);
  const std::vector<int64_t> off = readAll<int64_t>(a[1]);
  const std::vector<char> txt = readAll<char>(a[2]);
  const size_t n = events.size() / xm::XM_PILEUP_EVENT_WORDS, split = (size_t)atoll(a[3]);
  if (off.size() != n + 1 || split > n) { fprintf(stderr, "bad sizes\n"); return 2; }
  std::vector<long long> allEvents;
  std::vector<int64_t> allOff;
  std::vector<char> allText;
  xm::pileupAppendCall(events.data(), split, off.data(), txt.data(), allEvents, &allOff, &allText);
  xm::pileupAppendCall(events.data() + split * xm::XM_PILEUP_EVENT_WORDS, n - split, off.data() + split, txt.data(), allEvents, &allOff, &allText);
  writeAll(allEvents);
  writeAll(allOff);
  writeAll(allText);
  return 0;
}

int page(char** a) {
  const std::vector<int64_t> off = readAll<int64_t>(a[0]);
  printf("%lld\n", (long long)xm::pileupTextPage(off, (int64_t)off.size() - 1, atoll(a[1]), atoll(a[2]), atoll(a[3])));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "text" && argc == 7) return text(argv + 2);
  if (mode == "append" && argc == 6) return append(argv + 2);
  if (mode == "page" && argc == 6) return page(argv + 2);
  fprintf(stderr, "usage: pileup_text_main text MATE_OFF MATE_LEN CODES EVENTS QUERY_BASE | append EVENTS OFF TEXT SPLIT | page OFF FIRST N CAP\n");
  return 2;
}
