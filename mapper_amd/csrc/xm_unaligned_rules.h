// The unaligned-query file's text, once, as plain C++: what libxm_hostio.so's appendUnaligned (xm_hostio.cpp: the definition) writes for a
// query without an alignment - every mate as it came in, FASTQ where it came with qualities, else FASTA.  The kernels of xm_unaligned.h call these functions
// on the device (they are host+device there, and plain inline functions everywhere else); tests/unaligned_rules_main.cpp calls them on the host, so
// tests/test_unaligned_rules.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation, no library call.
//
// Whether a query is unaligned is xm_summary_rules.h's to say (summaryWalkQuery: no alignment in a slice that is well formed).  For such a query q every mate
// m < mateCount[q], in order, contributes
//   '@' if hasQual is non-null and hasQual[2q + m] is set, else '>'; the name; '\n'; the bases, decoded by code & 15 through ?ACMGRSVTWYHKDBN; '\n';
//   and for a FASTQ mate "+\n", the quality bytes, '\n'.
// A mate slot beyond mateCount[q] - the padding of a single read, of a split batch's section - is never written.
//
// A sink takes the text.  compose(f): f(char* p) writes at most XM_UNALIGNED_ROOM bytes at p and returns how many; spread(n, byteAt): n bytes, byte i =
// byteAt(i).  xm_sam.h's SamTileSink is such a sink (a wavefront's tile), the test program has one that appends to a string.  A record's size is a closed form
// of the lengths (unalignedRecordBytes), so nothing is walked to measure it.  Every load is clipped to the batch's arrays, whatever the offsets say: a byte
// outside of them reads as '?' (codes: code 0), and a length that is negative counts as 0 - in the size and in the text alike.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_UNALIGNED_FN __host__ __device__ inline
#else
#define XM_UNALIGNED_FN inline
#endif

namespace xm {

constexpr int XM_UNALIGNED_ROOM = 4;  // the most one compose() writes ("\n+\n" is the longest)

// the batch: xm_query_batch's arrays and xmio_batch's names and qualities (nameOff and qualOff have 2 * nq + 1 entries; quals / qualOff / hasQual may be
// null: a batch without qualities), with the bytes each array holds
struct UnalignedBatch {
  int64_t nq;
  const int32_t* mateCount; const int64_t* mateOffset; const int32_t* mateLength;
  const uint8_t* codes; int64_t codesLength;
  const char* names; const int64_t* nameOff; int64_t namesLength;
  const char* quals; const int64_t* qualOff; const uint8_t* hasQual; int64_t qualsLength;
};

XM_UNALIGNED_FN char unalignedBase(int code) { return "?ACMGRSVTWYHKDBN"[code & 15]; }

// one mate slot's three fields as the text shows them
struct UnalignedMate {
  bool fastq;
  long long nameAt, nameLen, codesAt, bases, qualAt, qualLen;
};

XM_UNALIGNED_FN long long unalignedSpan(long long lo, long long hi) { return hi > lo ? hi - lo : 0; }

XM_UNALIGNED_FN UnalignedMate unalignedMate(const UnalignedBatch& b, long long slot) {
  UnalignedMate m;
  m.fastq = b.hasQual != nullptr && b.quals != nullptr && b.qualOff != nullptr && b.hasQual[slot] != 0;
  m.nameAt = b.nameOff[slot];
  m.nameLen = unalignedSpan(m.nameAt, b.nameOff[slot + 1]);
  m.codesAt = b.mateOffset[slot];
  m.bases = b.mateLength[slot] > 0 ? b.mateLength[slot] : 0;
  m.qualAt = m.fastq ? b.qualOff[slot] : 0;
  m.qualLen = m.fastq ? unalignedSpan(m.qualAt, b.qualOff[slot + 1]) : 0;
  return m;
}

XM_UNALIGNED_FN int unalignedMates(const UnalignedBatch& b, long long q) {
  const int n = b.mateCount[q];
  return n < 0 ? 0 : (n > 2 ? 2 : n);
}

// the bytes of query q's record
XM_UNALIGNED_FN long long unalignedRecordBytes(const UnalignedBatch& b, long long q) {
  long long bytes = 0;
  const int n = unalignedMates(b, q);
  for (int mate = 0; mate < n; mate++) {
    const UnalignedMate m = unalignedMate(b, 2 * q + mate);
    bytes += 1 + m.nameLen + 1 + m.bases + 1 + (m.fastq ? 2 + m.qualLen + 1 : 0);
  }
  return bytes;
}

// byte i of a text array from `at` on, clipped to the array
struct UnalignedTextAt {
  const char* p; long long at, length;
  XM_UNALIGNED_FN char operator()(long long i) const {
    const long long k = at + i;
    return k >= 0 && k < length ? p[k] : '?';
  }
};
// base i of a mate, clipped to the codes
struct UnalignedBasesAt {
  const uint8_t* codes; long long at, length;
  XM_UNALIGNED_FN char operator()(long long i) const {
    const long long k = at + i;
    return unalignedBase(k >= 0 && k < length ? codes[k] : 0);
  }
};
struct UnalignedPut1 { char a; XM_UNALIGNED_FN int operator()(char* p) const { p[0] = a; return 1; } };
struct UnalignedPut3 { XM_UNALIGNED_FN int operator()(char* p) const { p[0] = '\n'; p[1] = '+'; p[2] = '\n'; return 3; } };

// query q's record -> sink, mates(q) the number of mates written
template <class Sink>
XM_UNALIGNED_FN int unalignedWriteQuery(const UnalignedBatch& b, long long q, Sink& sink) {
  const int n = unalignedMates(b, q);
  for (int mate = 0; mate < n; mate++) {
    const UnalignedMate m = unalignedMate(b, 2 * q + mate);
    sink.compose(UnalignedPut1{m.fastq ? '@' : '>'});
    sink.spread(m.nameLen, UnalignedTextAt{b.names, m.nameAt, b.namesLength});
    sink.compose(UnalignedPut1{'\n'});
    sink.spread(m.bases, UnalignedBasesAt{b.codes, m.codesAt, b.codesLength});
    if (m.fastq) {
      sink.compose(UnalignedPut3{});
      sink.spread(m.qualLen, UnalignedTextAt{b.quals, m.qualAt, b.qualsLength});
    }
    sink.compose(UnalignedPut1{'\n'});
  }
  return n;
}

}  // namespace xm
