// The count behind --out-refs-map-count as plain C++: per aligned query the set of contigs its alignments lie on - ObjectSink.write in
// mapper_amd/cli.py is the definition: {contig of sa for comp in comps for al in comp for sa in al.components}, counted only for queries with an alignment.
// The kernels of xm_refs.h call these functions on the device (they are host+device there, and plain inline functions everywhere else);
// tests/refs_rules_main.cpp calls them on the host, so tests/test_refs_rules.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no
// allocation, no library call.  Contig names and their order are the host's business: here a contig is its index.
//
// The walk of a slice and what makes one malformed is xm_result_walk.h's; the visitor here looks at no block and at no double.
#pragma once
#include "xm_result_walk.h"

#if defined(__HIPCC__)
#define XM_REFS_FN __host__ __device__ inline
#else
#define XM_REFS_FN inline
#endif

namespace xm {

constexpr int XM_REFS_INLINE = 8;  // distinct contigs of a query that a set holds; a query on more is `wide` and is left to the host

// What one query's slice says: whether it has an alignment, its sequence alignments, and the ascending distinct contigs of them (ids[0 .. n)), unless there
// are more than XM_REFS_INLINE: then wide is set and ids, n mean nothing.
struct RefSet {
  bool aligned = false, wide = false;
  int32_t nSeq = 0, n = 0;
  int32_t ids[XM_REFS_INLINE] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// contig c joins the set (constant indices only: on the device the set stays in registers)
XM_REFS_FN void refsInsert(RefSet& s, int32_t c) {
  if (s.wide) return;
  bool found = false;
  int pos = 0;
  for (int i = 0; i < XM_REFS_INLINE; i++)
    if (i < s.n) { found = found || s.ids[i] == c; pos += s.ids[i] < c ? 1 : 0; }
  if (found) return;
  if (s.n == XM_REFS_INLINE) { s.wide = true; return; }
  for (int i = XM_REFS_INLINE - 1; i > 0; i--)
    if (i > pos && i <= s.n) s.ids[i] = s.ids[i - 1];
  for (int i = 0; i < XM_REFS_INLINE; i++)
    if (i == pos) s.ids[i] = c;
  s.n++;
}

// The sink that keeps nothing: contig(k, c) gets the contig of sequence alignment k = 0, 1, ... in stream order.
struct RefsNoContigs {
  XM_REFS_FN void contig(long long, int32_t) {}
};

// The visitor that collects: every sequence's contig to the sink and into the set.
template <class Sink>
struct RefsCollect {
  RefSet s;
  Sink& sink;
  XM_WALK_FN void take(int32_t contig) {
    sink.contig(s.nSeq, contig);
    refsInsert(s, contig);
    s.nSeq++;  // (a slice's length is an int32, and a sequence alignment takes seven ints: no overflow)
  }
  XM_WALK_FN bool operator()(const ResultAlignment& al) {
    take(al.first.contig);
    if (al.nseq == 2) take(al.second.contig);
    s.aligned = true;
    return true;
  }
};

// Query q's slice -> out; sink.contig(k, contig) for every sequence alignment in stream order, repeats included.  false: the slice is malformed
// (xm_result_walk.h), and out is untouched (the sink may have seen the contigs of the alignments in front of the fault).
template <class Sink>
XM_REFS_FN bool refsWalkQuery(const ResultStreams& st, long long q, RefSet& out, Sink& sink) {
  RefsCollect<Sink> collect{RefSet(), sink};
  if (!resultWalkQuery(st, q, collect)) return false;
  out = collect.s;
  return true;
}

XM_REFS_FN bool refsWalkQuery(const ResultStreams& st, long long q, RefSet& out) {
  RefsNoContigs none;
  return refsWalkQuery(st, q, out, none);
}

XM_REFS_FN unsigned long long refsMix(unsigned long long z) {  // SplitMix64's finaliser
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 64 bits over (n, ids[0 .. n)); only the low `bits` of them when bits < 64 (a test knob: few bits make collisions); never 0, which marks an empty slot.
// The fingerprint decides how many queries are left to the host, never the output.
XM_REFS_FN unsigned long long refsFingerprint(const int32_t* ids, int n, int bits) {
  unsigned long long h = refsMix((unsigned long long)(unsigned)n + 0x9E3779B97F4A7C15ull);
  for (int i = 0; i < XM_REFS_INLINE; i++)
    if (i < n) h = refsMix(h ^ refsMix((unsigned long long)(uint32_t)ids[i] + 0xD1B54A32D192ED03ull * (unsigned long long)(i + 1)));
  if (bits >= 0 && bits < 64) h &= (1ull << bits) - 1;
  return h == 0 ? 1 : h;
}

XM_REFS_FN bool refsSame(const RefSet& a, const RefSet& b) {
  if (a.wide || b.wide || a.n != b.n) return false;
  bool same = true;
  for (int i = 0; i < XM_REFS_INLINE; i++)
    if (i < a.n && a.ids[i] != b.ids[i]) same = false;
  return same;
}

}  // namespace xm
