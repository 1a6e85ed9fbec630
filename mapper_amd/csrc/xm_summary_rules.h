// What the host still needs of a batch's result streams once the SAM text is made elsewhere, once, as plain C++: the statistics that
// libxm_hostio.so's xmio_write_batch counts with sam_fd = -1 (xm_hostio.cpp, formatRange with wantSam off and the penalty loop: the definition) - whether a
// query is aligned, its alignments, the aligned length and the indels of their blocks, and every alignment's totalPenalty in stream order.  The kernels of
// xm_summary.h call these functions on the device (they are host+device there, and plain inline functions everywhere else); tests/summary_rules_main.cpp
// calls them on the host, so tests/test_summary_rules.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation, no library call.
//
// Why a second walker beside samWalkQuery (xm_sam_rules.h) and not a sink for it: samWalkQuery reads the batch (mate counts, lengths, names) and rejects
// what only a SAM record cannot express (mate >= nMates, a paired alignment of one sequence), which formatRange accepts when it writes no SAM; and a sink
// sees text, not blocks.  The walk below needs neither the batch nor the contig names, and its checks are formatRange's with wantSam off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_SUMMARY_FN __host__ __device__ inline
#else
#define XM_SUMMARY_FN inline
#endif

namespace xm {

// the four result streams (include/xmapper_hip.h:73-82) and the number of contigs of the index
struct SummaryStreams { const int32_t* ints; const double* dbls; const int64_t* intOff; const int64_t* dblOff; int32_t numContigs; };

// what one query adds to the statistics
struct QuerySummary {
  long long aligned = 0, alignments = 0, alignedLength = 0, indels = 0;
};

// The sink that only counts: penalty(a, p) gets alignment a's totalPenalty.
struct SummaryNoPenalties {
  XM_SUMMARY_FN void penalty(long long, double) {}
};

// Query q's slice of the two streams -> out; sink.penalty(a, totalPenalty) for alignment a = 0, 1, ... in stream order.  false: the slice is malformed -
// exactly where formatRange returns false with wantSam off (nseq outside 1 .. 2, nb < 1, a contig outside [0, numContigs), the cursor past the slice's
// end) - and nothing in out or the sink counts.  Unlike the host code, no int is read at or behind the end of q's slice of the int stream and no double at
// or behind the end of its slice of the other: a slice that ends early is malformed.
template <class Sink>
XM_SUMMARY_FN bool summaryWalkQuery(const SummaryStreams& st, long long q, QuerySummary& out, Sink& sink) {
  const int32_t* ints = st.ints;
  long long at = st.intOff[q];
  const long long end = st.intOff[q + 1];
  long long dat = st.dblOff[q];
  const long long dend = st.dblOff[q + 1];
  QuerySummary s;
  if (at >= end) return false;
  const int ncomp = ints[at++];
  for (int c = 0; c < ncomp; c++) {
    if (at >= end) return false;
    const int nal = ints[at++];
    for (int a = 0; a < nal; a++) {
      if (at + 2 > end || dat + 4 > dend) return false;
      const int nseq = ints[at + 1];  // ([at]: innerDistance)
      at += 2;
      const double penalty = st.dbls[dat + 3];
      dat += 4;
      if (nseq < 1 || nseq > 2) return false;
      for (int k = 0; k < nseq; k++) {
        if (at + 3 > end || dat + 2 > dend) return false;
        const int32_t contig = ints[at], nb = ints[at + 2];
        if (nb < 1 || contig < 0 || contig >= st.numContigs) return false;
        const long long blocks = at + 3;
        at += 3 + 4ll * nb;
        dat += 2;
        if (at > end) return false;
        for (int j = 0; j < nb; j++) {
          const int32_t la = ints[blocks + 4ll * j + 2], lb = ints[blocks + 4ll * j + 3];
          s.alignedLength += la;
          if (la != lb) s.indels++;
        }
      }
      sink.penalty(s.alignments, penalty);
      s.alignments++;
    }
  }
  s.aligned = s.alignments > 0 ? 1 : 0;
  out = s;
  return true;
}

}  // namespace xm
