// The host's side of the confidence table (IndexView::conf): the open-addressing table the kernels read with confLookup (xm_defs.h), the settings its
// values were computed for, and which query lengths it was seeded for.  Plain C++: no GPU in here; the context (xm_capi.hip) copies data() to the
// device when dirty() and inserts the keys the kernels missed.
#pragma once
#include "xm_defs.h"
#include "xm_confidence.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_set>
#include <vector>

namespace xm {

class ConfTable {
  std::vector<ConfEntry> entries;           // power-of-two size, at most half full, linear probing from confHash
  size_t count = 0;
  struct { double maxPenaltySpan, mutationPenalty, granularity; int64_t totalSize; } sig = {0, 0, 0, 0};  // what the values depend on besides the key
  std::unordered_set<int32_t> seeded;       // query lengths whose whole-substitution sums are in the table
  double seedRate = -1;                     // (... for this MaxErrorRate)
  bool isDirty = true;                      // the device's copy is not this one
  static constexpr size_t kInitialSize = (size_t)1 << 14;

 public:
  // the value of (penalty, qlen) under the settings of the last prepare(), added if it is not there -> false: already there
  bool insert(double penalty, int32_t qlen) {
    uint64_t bits;
    memcpy(&bits, &penalty, 8);
    if ((count + 1) * 2 > entries.size()) {  // grow (and rehash) at half load
      std::vector<ConfEntry> old;
      old.swap(entries);
      entries.assign(old.empty() ? kInitialSize : old.size() * 2, ConfEntry{0, 0, 0, 0.0});
      for (const ConfEntry& e : old) if (e.used) { uint32_t h = confHash(e.penaltyBits, e.queryLength) & mask(); while (entries[h].used) h = (h + 1) & mask(); entries[h] = e; }
    }
    uint32_t h = confHash(bits, qlen) & mask();
    while (entries[h].used) {
      if (entries[h].penaltyBits == bits && entries[h].queryLength == qlen) return false;
      h = (h + 1) & mask();
    }
    entries[h] = ConfEntry{bits, qlen, 1, confidenceLengthOnHost(penalty, qlen, sig.maxPenaltySpan, sig.mutationPenalty, sig.granularity, sig.totalSize)};
    count++;
    isDirty = true;
    return true;
  }
  // the table for one align call: emptied when the settings it depends on changed; seeded with what the batch's reads will ask for in the common case
  // (an alignment without indels costs a whole number of substitutions: the sums 0, m, m + m, ... up to the allowed penalty), whatever else
  // comes up (ambiguity and unaligned penalties, spacing penalties of pairs, other sums) is inserted after the pass that missed it.
  // lens: the batch's distinct query lengths, ascending.  A length is seeded once; a call seeds at most seedBudget entries (fixed-length batches: a few
  // dozen; a batch of unsplit long reads has thousands of distinct lengths with thousands of sums each, of which the reads ask for a few: what is
  // not seeded comes in through the miss path; 0: nothing is seeded).
  void prepare(const Params& p, const std::vector<int32_t>& lens, double granularity, int64_t totalSize, long long seedBudget) {
    const decltype(sig) now = {p.Max_PenaltySpan, p.MutationPenalty, granularity, totalSize};
    if (memcmp(&now, &sig, sizeof(sig)) != 0) { sig = now; entries.clear(); count = 0; isDirty = true; seeded.clear(); }
    if (seedRate != p.MaxErrorRate) { seedRate = p.MaxErrorRate; seeded.clear(); }
    if (entries.empty()) entries.assign(kInitialSize, ConfEntry{0, 0, 0, 0.0});
    for (int32_t len : lens) {
      if (seeded.count(len)) continue;
      const double limit = (double)len * p.MaxErrorRate + p.Max_PenaltySpan + p.MutationPenalty;
      const double steps = p.MutationPenalty > 0 ? std::min(4096.0, std::floor(limit / p.MutationPenalty) + 2) : 1;
      if (steps > (double)seedBudget) continue;
      seedBudget -= (long long)steps;
      double pen = 0;
      for (int j = 0; j < (int)steps && pen <= limit; j++) { insert(pen, len); pen += p.MutationPenalty; }
      seeded.insert(len);
    }
  }
  const ConfEntry* data() const { return entries.data(); }
  size_t size() const { return entries.size(); }      // slots
  size_t used() const { return count; }
  uint32_t mask() const { return (uint32_t)(entries.size() - 1); }
  bool dirty() const { return isDirty; }
  void markUploaded() { isDirty = false; }
};

}  // namespace xm
