// A query's slice of the result streams, walked in one place, as plain C++: the layout that an align call leaves in HBM
// (include/xmapper_hip.h:73-106) and the rules that make a slice malformed - libxm_hostio.so's formatRange (xm_hostio.cpp: the definition) with wantSam off.
// The SAM records (xm_sam_rules.h), the batch summary and the unaligned-query file (xm_summary_rules.h) and the reference counts (xm_refs_rules.h) are
// visitors of this walk, so they reject exactly the same slices.  Host+device under hipcc, plain inline functions everywhere else; no HIP, no threads,
// no allocation, no library call.
//
// The slice of query q, ints[intOff[q] .. intOff[q + 1]) beside dbls[dblOff[q] .. dblOff[q + 1]):
//   ncomp, then per component: nal, then per alignment: innerDistance, nseq and four doubles (spacingPenalty, .., .., totalPenalty), then per sequence:
//   contig, reversed, nb and two doubles, then nb blocks of four ints (queryStart, refStart, queryLength, refLength).
// Malformed, in the order the walk meets them:
//   the int cursor at or behind the slice's end in front of ncomp or of a component's nal
//   fewer than two ints or four doubles left in front of an alignment
//   nseq outside 1 .. 2
//   fewer than three ints or two doubles left in front of a sequence
//   nb < 1, a contig outside [0, numContigs)
//   the int cursor behind the slice's end behind a sequence's blocks
//   whatever the visitor refuses.
// Unlike the host code, no int is read at or behind the end of q's slice of the int stream and no double at or behind the end of its slice of the other: a
// slice that ends early is malformed.  What is left of a slice behind its last component is not looked at.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_WALK_FN __host__ __device__ __forceinline__
#else
#define XM_WALK_FN inline
#endif

namespace xm {

constexpr unsigned long long XM_NO_QUERY = ~0ull;  // a stage's control word for "the lowest query that ..." while there is none

// the four result streams where they lie (include/xmapper_hip.h:73-82) and the number of contigs of the index
struct ResultStreams { const int32_t* ints; const double* dbls; const int64_t* intOff; const int64_t* dblOff; int32_t numContigs; };
using SamStreams = ResultStreams;      // the two names from before the streams had one struct: the stand-alone test programs of the rules say them
using SummaryStreams = ResultStreams;  // (SamStreams had no numContigs: the SAM walk takes its bound from SamContigs::num)

// One sequence of an alignment where it lies in the int stream: (contig, reversed, nb) at `at`, the nb blocks behind them.  The walk has loaded contig and nb.
struct ResultSeq {
  const int32_t* at;
  int32_t contig, nb;
  XM_WALK_FN const int32_t* blocks() const { return at + 3; }
};

// One alignment whose sequences have passed every rule above, as a visitor gets it.  The walk has loaded the counts and, per sequence, contig and nb - no
// block and no double: a visitor loads what it needs, all of it inside the slice.
struct ResultAlignment {
  int comp, ncomp;         // the component, and how many the query has
  long long index;         // the alignment's running index within the query
  int nseq;                // 1 or 2: `second` means nothing with 1
  ResultSeq first, second;
  const double* dbls;      // the alignment's four doubles
};

// the sequence at the cursors -> s, and the cursors behind it; false: malformed
XM_WALK_FN bool resultTakeSeq(const ResultStreams& st, long long& at, long long end, long long& dat, long long dend, ResultSeq& s) {
  if (at + 3 > end || dat + 2 > dend) return false;
  s.at = st.ints + at; s.contig = st.ints[at]; s.nb = st.ints[at + 2];
  if (s.nb < 1 || s.contig < 0 || s.contig >= st.numContigs) return false;
  at += 3 + 4ll * s.nb;
  dat += 2;
  return at <= end;
}

// Query q's slice: visit(alignment) once per alignment in stream order, after both of its sequences have passed.  false: the slice is malformed - one of
// the rules above, or visit returned false - and whatever the visitor has seen in front of the fault does not count.
template <class Visitor>
XM_WALK_FN bool resultWalkQuery(const ResultStreams& st, long long q, Visitor& visit) {
  const int32_t* ints = st.ints;
  long long at = st.intOff[q];
  const long long end = st.intOff[q + 1];
  long long dat = st.dblOff[q];
  const long long dend = st.dblOff[q + 1];
  ResultAlignment al;
  al.index = 0;
  if (at >= end) return false;
  al.ncomp = ints[at++];
  for (al.comp = 0; al.comp < al.ncomp; al.comp++) {
    if (at >= end) return false;
    const int nal = ints[at++];
    for (int a = 0; a < nal; a++) {
      if (at + 2 > end || dat + 4 > dend) return false;
      al.nseq = ints[at + 1];  // ([at]: innerDistance)
      at += 2;
      al.dbls = st.dbls + dat;
      dat += 4;
      if (al.nseq < 1 || al.nseq > 2) return false;
      if (!resultTakeSeq(st, at, end, dat, dend, al.first)) return false;
      if (al.nseq == 2 && !resultTakeSeq(st, at, end, dat, dend, al.second)) return false;
      if (!visit(al)) return false;
      al.index++;
    }
  }
  return true;
}

}  // namespace xm
