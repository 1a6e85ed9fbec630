// The thresholds of the mutations file, once, as plain C++: what pileup.MatchDatabase.mutations() and pileup._below() - the definition - decide
// over the counts of a pile-up.  The kernels of xm_mutations.h call these functions on the device (they are host+device there, and plain inline functions
// everywhere else); tests/mutations_rules_main.cpp calls them on the host, so tests/test_mutations_rules.py checks without a GPU the very code the GPU runs.
// No HIP, no threads, no allocation, no library call.
//
// Counts are integers in units of 1 / XM_PILEUP_UNIT of a read base.  A depth becomes the double units / 1441440.0, as numpy divides a uint64 by the unit.  A
// threshold pair (total, fraction) drops what it is asked about when `total < minTotal` (doubles) or `(float)support < (float)fraction * (float)total` (the
// product taken in float32: 0.7 of a depth of 10 is 7.0 there, and an allele seen 7 times of 10 stays).  The total-depth thresholds are doubles: a caller that
// narrowed them to float32 (MutationDetectionParameters does) widens them without loss, one that did not is compared as the host compares it.
//
// A SNP row (position, letter b of ACGT) exists when alt[b][position] != 0 and the SNP pair does not drop it, the total being the depth at the position.
// An indel candidate (1-based pos1 in its contig, kind 1 insertion / 2 deletion, length n, support in units) looks at the middle depth of its own contig:
// at = clamp(pos1 - 1, 0, contigLen - 1); the start pair drops it over middle[at]; otherwise keep starts at 1 and grows while keep < n and the continuation
// pair does not drop the base at min(at + keep, contigLen - 1) (deletion) or at `at` (insertion).  No position leaves the candidate's contig.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_MUTATIONS_FN __host__ __device__ inline
#else
#define XM_MUTATIONS_FN inline
#endif

namespace xm {

constexpr double XM_MUTATIONS_UNIT = 1441440.0;  // XM_PILEUP_UNIT (include/xmapper_hip.h)

// MutationDetectionParameters: xm_mutation_filter's fields
struct MutationFilter {
  double minSNPTotalDepth, minIndelTotalStartDepth, minIndelContinuationTotalDepth;
  float minSNPDepthFraction, minIndelStartDepthFraction, minIndelContinuationDepthFraction;
  int32_t reserved;
};

XM_MUTATIONS_FN double mutationsDepth(unsigned long long units) { return (double)units / XM_MUTATIONS_UNIT; }

// pileup._below: support < fraction * total in float arithmetic
XM_MUTATIONS_FN bool mutationsBelow(double support, float fraction, double total) {
  const float product = fraction * (float)total;
  return (float)support < product;
}

// what a threshold pair drops
XM_MUTATIONS_FN bool mutationsDropped(double support, double total, double minTotal, float fraction) {
  return total < minTotal || mutationsBelow(support, fraction, total);
}

// a SNP row of `alt` units at a position of `depth` units
XM_MUTATIONS_FN bool mutationsSnpRow(unsigned long long alt, unsigned long long depth, const MutationFilter& f) {
  if (alt == 0) return false;
  return !mutationsDropped(mutationsDepth(alt), mutationsDepth(depth), f.minSNPTotalDepth, f.minSNPDepthFraction);
}

// An indel candidate over the middle depth of its contig (middle[0 .. contigLen), contigLen >= 1).  -> keep (0: dropped by the start pair); *totalUnits = the
// middle depth where it starts, also when it is dropped.
XM_MUTATIONS_FN long long mutationsJudgeIndel(const unsigned long long* middle, long long contigLen, long long pos1, int kind, long long n, unsigned long long supportUnits,
                                              const MutationFilter& f, unsigned long long* totalUnits) {
  const long long last = contigLen - 1;
  long long at = pos1 - 1;
  if (at < 0) at = 0;
  if (at > last) at = last;
  const unsigned long long start = middle[at];
  *totalUnits = start;
  const double support = mutationsDepth(supportUnits);
  if (mutationsDropped(support, mutationsDepth(start), f.minIndelTotalStartDepth, f.minIndelStartDepthFraction)) return 0;
  long long keep = 1;
  while (keep < n) {
    const long long here = kind == 2 ? (at + keep < last ? at + keep : last) : at;
    if (mutationsDropped(support, mutationsDepth(middle[here]), f.minIndelContinuationTotalDepth, f.minIndelContinuationDepthFraction)) break;
    keep++;
  }
  return keep;
}

// The contig of a global forward position: the last c with contigStart[c] <= position (contigStart has numContigs entries, ascending, the first 0).
XM_MUTATIONS_FN int mutationsContigOf(const int64_t* contigStart, int numContigs, long long position) {
  int lo = 0, hi = numContigs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)contigStart[mid] <= position) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace xm
