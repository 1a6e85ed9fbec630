// What the host still needs of a batch's result streams once the SAM text is made elsewhere, once, as plain C++: the statistics that
// libxm_hostio.so's xmio_write_batch counts with sam_fd = -1 (xm_hostio.cpp, formatRange with wantSam off and the penalty loop: the definition) - whether a
// query is aligned, its alignments, the aligned length and the indels of their blocks, and every alignment's totalPenalty in stream order.  The kernels of
// xm_summary.h call these functions on the device (they are host+device there, and plain inline functions everywhere else); tests/summary_rules_main.cpp
// calls them on the host, so tests/test_summary_rules.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation, no library call.
//
// The walk of a slice and what makes one malformed is xm_result_walk.h's; what is counted here is a visitor of it that reads the blocks' two lengths and one
// double per alignment.  The unaligned-query file (xm_unaligned.h) asks the same walk who is unaligned.
#pragma once
#include "xm_result_walk.h"

#if defined(__HIPCC__)
#define XM_SUMMARY_FN __host__ __device__ inline
#else
#define XM_SUMMARY_FN inline
#endif

namespace xm {

// what one query adds to the statistics
struct QuerySummary {
  long long aligned = 0, alignments = 0, alignedLength = 0, indels = 0;
};

// The sink that only counts: penalty(a, p) gets alignment a's totalPenalty.
struct SummaryNoPenalties {
  XM_SUMMARY_FN void penalty(long long, double) {}
};

// The visitor that counts: the aligned length and the indels of an alignment's blocks, and its totalPenalty to the sink.
template <class Sink>
struct SummaryCounts {
  QuerySummary s;
  Sink& sink;
  XM_WALK_FN void blocksOf(const ResultSeq& sa) {
    const int32_t* blocks = sa.blocks();
    for (int j = 0; j < sa.nb; j++) {
      const int32_t la = blocks[4ll * j + 2], lb = blocks[4ll * j + 3];
      s.alignedLength += la;
      if (la != lb) s.indels++;
    }
  }
  XM_WALK_FN bool operator()(const ResultAlignment& al) {
    blocksOf(al.first);
    if (al.nseq == 2) blocksOf(al.second);
    sink.penalty(al.index, al.dbls[3]);
    s.alignments++;
    return true;
  }
};

// Query q's slice of the two streams -> out; sink.penalty(a, totalPenalty) for alignment a = 0, 1, ... in stream order.  false: the slice is malformed
// (xm_result_walk.h), and nothing in out or the sink counts.
template <class Sink>
XM_SUMMARY_FN bool summaryWalkQuery(const ResultStreams& st, long long q, QuerySummary& out, Sink& sink) {
  SummaryCounts<Sink> counts{QuerySummary(), sink};
  if (!resultWalkQuery(st, q, counts)) return false;
  counts.s.aligned = counts.s.alignments > 0 ? 1 : 0;
  out = counts.s;
  return true;
}

}  // namespace xm
