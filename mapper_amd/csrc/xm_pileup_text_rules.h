// The text of an insertion event of the pile-up, once, as plain C++: which bases of which mate an event (include/xmapper_hip.h: eight
// int64) stands for, how many of them are kept, and how the host orders the events of one xm_pileup_add_last call and carries each event's text along.
// The definition is pileup.MatchDatabase.mutations: oriented = reverse_complement(mate) if reversed else mate; text = decode(oriented[startA : startA + length]).
// The kernels of xm_pileup_text.h call the first half on the device (host+device there, plain inline functions everywhere else); xm_pileup_add_last calls the
// second half; tests/pileup_text_main.cpp calls both on the host, so tests/test_pileup_text_rules.py checks without a GPU the very code the GPU runs.
// The 16 letters are xm_sam_rules.h's samBase (= api._DECODE): they are not stated again here.  No HIP, no threads, no library call on the device half.
#pragma once
#include "xm_sam_rules.h"
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace xm {

constexpr int XM_PILEUP_EVENT_WORDS = 8;  // contig, position, type (1 insertion, 2 deletion), length, query, mate | reversed << 1 | near end << 2, startA, weight

// Bytes of text kept for an event of `type` with `length` bases from startA on in a mate of readLen bases: clamp(min(length, readLen - startA), 0, length) -
// what the Python slice gives - and 0 for a deletion.  A startA in front of the mate keeps nothing (no event of the kernel has one; an event handed in may
// hold anything): whatever the four numbers are, [startA, startA + kept) lies inside the mate.
XM_SAM_FN long long pileupTextKept(long long type, long long length, long long startA, long long readLen) {
  if (type != 1 || length <= 0 || startA < 0 || startA >= readLen) return 0;
  const long long room = readLen - startA;
  return length < room ? length : room;
}
// byte i (0 <= i < kept) of the event's text; codes: the mate as given (as the FASTQ had it), reversed: bit 1 of the event's flags
XM_SAM_FN char pileupTextByte(const uint8_t* codes, int readLen, bool reversed, long long startA, long long i) { return samSeqBase(codes, readLen, reversed, (int)(startA + i)); }
XM_SAM_FN int pileupEventMate(long long flags) { return (int)(flags & 1); }
XM_SAM_FN bool pileupEventReversed(long long flags) { return ((flags >> 1) & 1) != 0; }

// ---------------------------------------------------------------- the host's half (plain functions: host only under hipcc)
// the order of the events of one call: (query ordinal, contig, position, flags, startA)
inline bool pileupEventBefore(const long long* a, const long long* b) {
  if (a[4] != b[4]) return a[4] < b[4];
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  if (a[5] != b[5]) return a[5] < b[5];
  return a[6] < b[6];
}
// The n events of a call as the device appended them (events: 8 words each; off, text: where each one's text lies, off has n + 1 entries - both null when
// no text is kept) are appended to allEvents in the order above; with text, every event's bytes follow it: allOff (one entry per event held, plus one;
// {0} when empty) and allText grow in the same order.
inline void pileupAppendCall(const long long* events, size_t n, const int64_t* off, const char* text, std::vector<long long>& allEvents, std::vector<int64_t>* allOff,
                             std::vector<char>* allText) {
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), (size_t)0);
  // (events that compare equal - two alignments of a query with the same block - keep the device's order; each one's text goes with it either way)
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pileupEventBefore(events + a * XM_PILEUP_EVENT_WORDS, events + b * XM_PILEUP_EVENT_WORDS); });
  const size_t at = allEvents.size();
  allEvents.resize(at + n * XM_PILEUP_EVENT_WORDS);
  for (size_t i = 0; i < n; i++) memcpy(allEvents.data() + at + i * XM_PILEUP_EVENT_WORDS, events + order[i] * XM_PILEUP_EVENT_WORDS, sizeof(long long) * XM_PILEUP_EVENT_WORDS);
  if (!off || !allOff || !allText) return;
  if (allOff->empty()) allOff->push_back(0);
  allText->reserve(allText->size() + (size_t)(off[n] - off[0]));
  for (size_t i = 0; i < n; i++) {
    const int64_t lo = off[order[i]], hi = off[order[i] + 1];
    allText->insert(allText->end(), text + lo, text + hi);
    allOff->push_back((int64_t)allText->size());
  }
}
// Paging of the kept text (xm_pileup_event_text): of the events [first, first + n) of `have`, as many as fit into cap bytes - at least one; -1 when the
// first one alone does not fit, or first is outside [0, have].  allOff as above.
inline int64_t pileupTextPage(const std::vector<int64_t>& allOff, int64_t have, int64_t first, int64_t n, int64_t cap) {
  if (first < 0 || first > have || cap < 0) return -1;
  int64_t m = n < have - first ? n : have - first;
  if (m <= 0) return 0;
  const int64_t base = allOff[(size_t)first];
  // the last event whose end is within cap bytes of the first one's start (the offsets never fall)
  const int64_t reach = cap > INT64_MAX - base ? INT64_MAX : base + cap;
  const auto end = std::upper_bound(allOff.begin() + first + 1, allOff.begin() + first + m + 1, reach);
  m = (int64_t)(end - (allOff.begin() + first + 1));
  return m > 0 ? m : -1;
}

}  // namespace xm
