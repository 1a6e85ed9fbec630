// The summary of a batch's result streams made on the GPU where an align call left them (included once, by xm_capi.hip): the kernels over the
// plain rules of xm_summary_rules.h.  Three stages, separate launches, no launch reads what another workgroup of the same launch wrote:
//   measure   a lane per query walks the query's slice: alignments[q] and unalignedFlag[q] (both 0 for a malformed slice); aligned queries, aligned length
//             and indels are summed over the wavefront by shuffles and added by its lane 0 to three 64-bit counters (integers: exact in any order); a
//             malformed slice leaves the lowest such query in the control word
//   offsets   exclusive sums of the two arrays in query order and both totals: the scan of xm_scan.h over the two int32 arrays
//   gather    a lane per query walks again and stores its alignments' penalties at penalties[off[q] + a] and, when it is unaligned and the list is wanted,
//             its index at unaligned[uoff[q]].  No lane stores outside its own [off[q], off[q + 1]) or behind the buffer's end, whatever the second walk yields.
// The double sum of the penalties is the host's: Mapper.run adds them in query order and the order is part of the result.
#pragma once
#include "xm_summary_rules.h"
#include <hip/hip_runtime.h>

namespace {

// ctl[0]: the lowest query with a malformed slice (xm::XM_NO_QUERY: none); ctl[1..3]: aligned queries, aligned length, indels
constexpr int XM_SUMMARY_CTL_WORDS = 4;

__device__ __forceinline__ long long summaryWaveSum(long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // (lane 0 holds the sum)
}

__global__ void __launch_bounds__(256) xm_summary_measure_kernel(xm::ResultStreams st, long long nq, int32_t* alignments, int32_t* unalignedFlag, unsigned long long* ctl) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  xm::QuerySummary s;
  if (q < nq) {  // (lanes behind the last query stay for the shuffles and add nothing)
    xm::SummaryNoPenalties none;
    const bool ok = xm::summaryWalkQuery(st, q, s, none);
    if (!ok) { atomicMin(&ctl[0], (unsigned long long)q); s = xm::QuerySummary(); }
    // (more alignments than an int32 holds cannot lie in a slice whose length is one: the arenas' per-query lengths are int32)
    alignments[q] = (int32_t)s.alignments;
    unalignedFlag[q] = ok && !s.aligned ? 1 : 0;
  }
  const long long aligned = summaryWaveSum(s.aligned), length = summaryWaveSum(s.alignedLength), indels = summaryWaveSum(s.indels);
  if ((threadIdx.x & 63) == 0) {
    if (aligned) atomicAdd(&ctl[1], (unsigned long long)aligned);
    if (length) atomicAdd(&ctl[2], (unsigned long long)length);
    if (indels) atomicAdd(&ctl[3], (unsigned long long)indels);
  }
}

// the sink of the gather: alignment a's penalty to out[lo + a], if that is inside the query's own range and the buffer
struct SummaryPenaltyStore {
  double* out;
  long long lo, hi, cap;
  __device__ void penalty(long long a, double p) {
    const long long at = lo + a;
    if (a >= 0 && at < hi && at < cap) out[at] = p;
  }
};

__global__ void __launch_bounds__(256) xm_summary_gather_kernel(xm::ResultStreams st, long long nq, const int64_t* off, const int64_t* uoff, double* penalties, long long penaltyCap,
                                                                int64_t* unaligned, long long unalignedCap) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const long long lo = off[q], hi = off[q + 1];
  if (hi > lo) {
    SummaryPenaltyStore sink{penalties, lo, hi, penaltyCap};
    xm::QuerySummary s;
    (void)xm::summaryWalkQuery(st, q, s, sink);
  }
  if (unaligned) {
    const long long u = uoff[q];
    if (uoff[q + 1] > u && u >= 0 && u < unalignedCap) unaligned[u] = q;
  }
}

}  // namespace
