// The rules of a SAM record, once, as plain C++: what libxm_hostio.so's formatter (xm_hostio.cpp, formatRange / appendCigar / appendSeq /
// javaDouble: the definition) writes for the result streams of a batch - the visitor of the walk of a query's slice (xm_result_walk.h) that makes the records, the
// fields of a record, Double.toString, and the byte length of a record and of a query.  The kernels of xm_sam.h call these functions on the device (they
// are host+device there, and plain inline functions everywhere else); tests/sam_rules_main.cpp calls them on the host, so tests/test_sam_rules.py checks
// without a GPU the very code the GPU runs.  No HIP, no threads, no allocation, no library call.
//
// The walk hands the text of a query to a SINK, in order.  A sink has
//   compose(f)          f(char* p) writes at most XM_SAM_ROOM bytes at p and returns how many (the flag, a position, one CIGAR operation, the tags ...)
//   bytesAt(p, n)       n bytes as they lie at p (a query name, a contig name)
//   seq(codes, n, rev)  n bases through samBase (rev: from the end, complemented)
//   endRecord()
// SamCount is the sink that only measures; xm_sam.h has the one that writes a wavefront's tile, the test program one that appends to a string.
#pragma once
#include "xm_result_walk.h"

#if defined(__HIPCC__)
#define XM_SAM_FN __host__ __device__ __forceinline__
#define XM_SAM_WALK __host__ __device__ inline
#else
#define XM_SAM_FN inline
#define XM_SAM_WALK inline
#endif

namespace xm {

constexpr int XM_SAM_ROOM = 64;           // the most one compose() writes ("\t*" + "\tcs:f:" + 24 + "\tAS:f:" + 24 + "\n" = 63 is the longest)
constexpr int XM_SAM_DOUBLE_BYTES = 24;   // the longest Double.toString: -1.2345678901234567E-308

// ---------------------------------------------------------------- powers of ten
// 10^k for k = XM_SAM_POW10_MIN .. XM_SAM_POW10_MAX as g * 2^(e2 - 127): g = the first 128 bits of 10^k, rounded up when bits were dropped, and
// e2 = floor(log2 10^k).  Computed here, by exact integer arithmetic on 32-bit limbs at compile time: 10^k for k >= 0 by multiplying by ten, 10^-m as
// floor(2^1200 / 10^m) by dividing by ten (floor(floor(x / 10) / 10) = floor(x / 100): the chain is exact), which 10^m never divides, so that rounding
// up is adding one.
constexpr int XM_SAM_POW10_MIN = -292, XM_SAM_POW10_MAX = 324, XM_SAM_POW10_COUNT = XM_SAM_POW10_MAX - XM_SAM_POW10_MIN + 1;
struct SamPow10Table {
  uint64_t hi[XM_SAM_POW10_COUNT], lo[XM_SAM_POW10_COUNT];
  int32_t e2[XM_SAM_POW10_COUNT];
};

namespace samdetail {
constexpr int LIMBS = 44;  // 1408 bits: 10^324 < 2^1077, and 2^1200
// bits [at, at + 32) of x
constexpr uint32_t limbAt(const uint32_t* x, int at) {
  const int w = at >> 5, s = at & 31;
  uint64_t v = x[w];
  if (w + 1 < LIMBS) v |= (uint64_t)x[w + 1] << 32;
  return (uint32_t)(v >> s);
}
// entry i of the table from x (top: its highest non-zero limb); ceilAlways: x stands for a value that is no integer, a little above x
constexpr void setEntry(SamPow10Table& t, int i, const uint32_t* x, int top, int scale, bool ceilAlways) {
  int bit = 31;
  while (!((x[top] >> bit) & 1u)) bit--;
  const int high = top * 32 + bit;  // position of the leading one
  uint64_t hi = 0, lo = 0;
  bool dropped = ceilAlways;
  if (high >= 127) {
    const int s = high - 127;
    lo = (uint64_t)limbAt(x, s) | ((uint64_t)limbAt(x, s + 32) << 32);
    hi = (uint64_t)limbAt(x, s + 64) | ((uint64_t)limbAt(x, s + 96) << 32);
    for (int w = 0; w < (s >> 5); w++) if (x[w]) dropped = true;
    if ((s & 31) && (x[s >> 5] & ((1u << (s & 31)) - 1u))) dropped = true;
  } else {  // (fewer than 128 bits: 10^k for k <= 38, exact) shifted up
    const int s = 127 - high;
    uint32_t y[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w <= top; w++) {
      const uint64_t v = (uint64_t)x[w] << (s & 31);
      y[w + (s >> 5)] |= (uint32_t)v;
      y[w + (s >> 5) + 1] |= (uint32_t)(v >> 32);
    }
    lo = (uint64_t)y[0] | ((uint64_t)y[1] << 32);
    hi = (uint64_t)y[2] | ((uint64_t)y[3] << 32);
  }
  if (dropped) { lo++; if (lo == 0) hi++; }
  t.hi[i] = hi; t.lo[i] = lo; t.e2[i] = high - scale;
}
}  // namespace samdetail

constexpr SamPow10Table makeSamPow10() {
  using namespace samdetail;
  SamPow10Table t{};
  uint32_t x[LIMBS] = {};
  x[0] = 1;
  int top = 0;
  for (int k = 0; k <= XM_SAM_POW10_MAX; k++) {
    setEntry(t, k - XM_SAM_POW10_MIN, x, top, 0, false);
    uint64_t carry = 0;
    for (int w = 0; w <= top; w++) { const uint64_t v = (uint64_t)x[w] * 10u + carry; x[w] = (uint32_t)v; carry = v >> 32; }
    if (carry) x[++top] = (uint32_t)carry;
  }
  for (int w = 0; w < LIMBS; w++) x[w] = 0;
  x[37] = 1u << 16;  // 2^1200
  top = 37;
  for (int m = 1; m <= -XM_SAM_POW10_MIN; m++) {
    uint64_t rem = 0;
    for (int w = top; w >= 0; w--) { const uint64_t v = (rem << 32) | x[w]; x[w] = (uint32_t)(v / 10u); rem = v % 10u; }
    if (!x[top]) top--;
    setEntry(t, -m - XM_SAM_POW10_MIN, x, top, 1200, true);
  }
  return t;
}
#if defined(__HIPCC__)
__device__ __constant__ const SamPow10Table kSamPow10Device = makeSamPow10();
#endif
inline constexpr SamPow10Table kSamPow10 = makeSamPow10();

XM_SAM_FN const SamPow10Table& samPow10() {
#if defined(__HIP_DEVICE_COMPILE__)
  return kSamPow10Device;
#else
  return kSamPow10;
#endif
}

// ---------------------------------------------------------------- Double.toString
XM_SAM_FN uint64_t samMulHi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the first 64 bits of g * cp (g = hi:lo, 128 bits; the product has 192), with every bit below them folded into the last one: enough to compare the
// product with a multiple of four exactly (round to odd)
XM_SAM_FN uint64_t samRoundToOdd(uint64_t hi, uint64_t lo, uint64_t cp) {
  const uint64_t x1 = samMulHi(lo, cp);
  const uint64_t y0 = hi * cp, y1 = samMulHi(hi, cp);
  const uint64_t z0 = y0 + x1, z1 = y1 + (z0 < x1 ? 1u : 0u);
  return z1 | (z0 > 1 ? 1u : 0u);
}

// floor(log10(2^e)) and floor(log10(3/4 * 2^e)) for |e| <= 1100: 1262611 = floor(2^22 * log10(2)), 524031 = floor(-2^22 * log10(3/4))
// (tests/sam_rules_main.cpp compares both with the table's e2 over the whole range of a double's exponents)
XM_SAM_FN int samFloorLog10Pow2(int e) { return (int)(((long long)e * 1262611) >> 22); }
XM_SAM_FN int samFloorLog10ThreeQuartersPow2(int e) { return (int)(((long long)e * 1262611 - 524031) >> 22); }

// The shortest decimal digits * 10^exp10 that reads back as the finite, non-zero double with these bits (its sign aside), and of the shortest ones the
// closest: Schubfach (R. Giulietti, "The Schubfach way to render doubles").  c * 2^q is the value; the interval of the decimals that round to it is scaled by
// 10^-k so that its width is between 1 and 10 ... and the candidates are the integers (and the multiples of ten) inside it.
XM_SAM_FN void samShortest(uint64_t bits, uint64_t& digits, int& exp10) {
  const uint64_t frac = bits & ((1ull << 52) - 1);
  const int biased = (int)((bits >> 52) & 0x7FF);
  const uint64_t c = biased ? (frac | (1ull << 52)) : frac;
  const int q = biased ? biased - 1075 : -1074;
  const bool even = (c & 1) == 0;
  const bool lowerCloser = frac == 0 && biased > 1;  // a power of two: the double below is half as far away
  const uint64_t cbl = 4 * c - 2 + (lowerCloser ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
  const int k = lowerCloser ? samFloorLog10ThreeQuartersPow2(q) : samFloorLog10Pow2(q);
  const SamPow10Table& t = samPow10();
  const int i = -k - XM_SAM_POW10_MIN;
  const int h = q + t.e2[i] + 1;  // 1 .. 4
  const uint64_t ghi = t.hi[i], glo = t.lo[i];
  const uint64_t vbl = samRoundToOdd(ghi, glo, cbl << h), vb = samRoundToOdd(ghi, glo, cb << h), vbr = samRoundToOdd(ghi, glo, cbr << h);
  const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
  const uint64_t s = vb / 4;
  if (s >= 10) {  // a multiple of ten in the interval is shorter than any other integer in it
    const uint64_t sp = s / 10;
    const bool upIn = lower <= 40 * sp, wpIn = 40 * sp + 40 <= upper;
    if (upIn != wpIn) { digits = sp + (wpIn ? 1 : 0); exp10 = k + 1; return; }
  }
  const bool uIn = lower <= 4 * s, wIn = 4 * s + 4 <= upper;
  if (uIn != wIn) { digits = s + (wIn ? 1 : 0); exp10 = k; return; }
  const uint64_t mid = 4 * s + 2;  // both or neither: the closer one, the even one on a tie
  const bool up = vb > mid || (vb == mid && (s & 1));
  digits = s + (up ? 1 : 0); exp10 = k;
}

XM_SAM_FN int samPutText(char* out, const char* s) {
  int n = 0;
  while (s[n]) { out[n] = s[n]; n++; }
  return n;
}

// v in decimal at out (at most 20 digits and a sign) -> bytes written
XM_SAM_FN int samPutInt(char* out, long long v) {
  char tmp[20];
  int n = 0, at = 0;
  unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
  if (v < 0) out[at++] = '-';
  do { tmp[n++] = (char)('0' + (int)(u % 10)); u /= 10; } while (u);
  while (n) out[at++] = tmp[--n];
  return at;
}

// Double.toString as xm_hostio.cpp's javaDouble has it, at out -> bytes written (at most XM_SAM_DOUBLE_BYTES): plain notation with at least one fractional
// digit for 1e-3 <= |x| < 1e7, otherwise d.dddE<n>; 0.0 also for -0.0
XM_SAM_FN int samPutDouble(char* out, double x) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, 8);
  const bool neg = (bits >> 63) != 0;
  const uint64_t mag = bits & ~(1ull << 63);
  if (mag > (0x7FFull << 52)) return samPutText(out, "NaN");
  if (mag == 0) return samPutText(out, "0.0");
  if (mag == (0x7FFull << 52)) return samPutText(out, neg ? "-Infinity" : "Infinity");
  uint64_t digits;
  int e;
  samShortest(mag, digits, e);
  while (digits % 10 == 0) { digits /= 10; e++; }
  char d[20];
  int n = 0;
  { char tmp[20]; uint64_t u = digits; do { tmp[n++] = (char)('0' + (int)(u % 10)); u /= 10; } while (u); for (int j = 0; j < n; j++) d[j] = tmp[n - 1 - j]; }
  const int exp10 = e + n - 1;  // of the first digit
  int at = 0;
  if (neg) out[at++] = '-';
  double a;
  __builtin_memcpy(&a, &mag, 8);
  if (a >= 1e-3 && a < 1e7) {
    if (exp10 >= 0) {
      const int intDigits = exp10 + 1;
      if (n <= intDigits) {
        for (int j = 0; j < n; j++) out[at++] = d[j];
        for (int j = n; j < intDigits; j++) out[at++] = '0';
        out[at++] = '.'; out[at++] = '0';
      } else {
        for (int j = 0; j < intDigits; j++) out[at++] = d[j];
        out[at++] = '.';
        for (int j = intDigits; j < n; j++) out[at++] = d[j];
      }
    } else {
      out[at++] = '0'; out[at++] = '.';
      for (int j = 0; j < -exp10 - 1; j++) out[at++] = '0';
      for (int j = 0; j < n; j++) out[at++] = d[j];
    }
  } else {
    out[at++] = d[0];
    out[at++] = '.';
    if (n > 1) for (int j = 1; j < n; j++) out[at++] = d[j]; else out[at++] = '0';
    out[at++] = 'E';
    at += samPutInt(out + at, exp10);
  }
  return at;
}

// ---------------------------------------------------------------- the record
XM_SAM_FN char samBase(int code) { return "?ACMGRSVTWYHKDBN"[code & 15]; }
XM_SAM_FN int samComplement(int b) { return ((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3); }
// base i of the SEQ field of a mate of n codes
XM_SAM_FN char samSeqBase(const uint8_t* codes, int n, bool rev, int i) { return rev ? samBase(samComplement(codes[n - 1 - i] & 15)) : samBase(codes[i]); }

// the batch (xm_query_batch's arrays and xmio_batch's names: name_off has 2 * nq + 1 entries) and the contig names one behind the other (off has num + 1
// entries; a contig of a record is one of these names, so num is the walk's bound, whatever the streams' own count says)
struct SamBatch {
  int64_t nq;
  const int32_t* mateCount; const int64_t* mateOffset; const int32_t* mateLength; const uint8_t* codes;
  const char* names; const int64_t* nameOff;
};
struct SamContigs { int32_t num; const char* names; const int64_t* off; };

// one sequence of an alignment where it lies in the int stream: (contig, reversed, nb) at `at`, the blocks behind
struct SamSeq { int32_t contig, rev, nb; const int32_t* blocks; };

// The sink that measures.
struct SamCount {
  long long bytes = 0, records = 0;
  template <class F> XM_SAM_FN void compose(F f) { char room[XM_SAM_ROOM]; bytes += f(room); }
  XM_SAM_FN void bytesAt(const char*, long long n) { bytes += n; }
  XM_SAM_FN void seq(const uint8_t*, int n, bool) { bytes += n; }
  XM_SAM_FN void endRecord() { records++; }
};

// the CIGAR of one sequence (xm_hostio.cpp appendCigar): soft clips at both ends, runs of the same operation merged
template <class Sink>
XM_SAM_WALK void samCigar(const SamSeq& sa, int queryLen, Sink& sink) {
  const int32_t* last = sa.blocks + 4 * (sa.nb - 1);
  const int lead = sa.blocks[0];
  if (lead > 0) sink.compose([&](char* p) { int n = samPutInt(p, lead); p[n++] = 'S'; return n; });
  char prevOp = 0;
  long long prevN = 0;
  for (int k = 0; k <= sa.nb; k++) {
    char op = 0;
    long long n = 0;
    if (k < sa.nb) {
      const int32_t la = sa.blocks[4 * k + 2], lb = sa.blocks[4 * k + 3];
      if (la == lb) { op = 'M'; n = la; } else if (lb == 0) { op = 'I'; n = la; } else { op = 'D'; n = lb; }
    }
    if (prevOp == op) { prevN += n; continue; }
    if (prevOp) sink.compose([&](char* p) { int m = samPutInt(p, prevN); p[m++] = prevOp; return m; });
    prevOp = op; prevN = n;
  }
  const int tail = queryLen - (last[0] + last[2]);
  if (tail > 0) sink.compose([&](char* p) { int n = samPutInt(p, tail); p[n++] = 'S'; return n; });
}

// The visitor that turns an alignment of query q into its records (one per sequence), in formatRange's order.  What only a SAM record cannot express
// is refused here, where formatRange returns false when it writes SAM: mate >= nMates (with that, the third component of a pair) and a paired
// single-component alignment with nseq != 2.
template <class Sink>
struct SamRecords {
  const SamBatch& b;
  const SamContigs& contigs;
  long long q;
  Sink& sink;
  XM_SAM_FN bool operator()(const ResultAlignment& al) {
    const int nMates = b.mateCount[q];
    const bool paired = nMates > 1;
    const int ncomp = al.ncomp, nseq = al.nseq;
    const double* dbls = al.dbls;  // (spacingPenalty, .., .., totalPenalty: loaded where they are written)
    SamSeq sas[2];
    sas[0] = SamSeq{al.first.contig, al.first.at[1], al.first.nb, al.first.blocks()};
    if (nseq == 2) sas[1] = SamSeq{al.second.contig, al.second.at[1], al.second.nb, al.second.blocks()};
    for (int k = 0; k < nseq; k++) {
      const SamSeq& sa = sas[k];
      const int mate = ncomp == 1 ? k : al.comp;  // (a pair that fell back to unpaired alignments: one component per mate)
      if (mate >= nMates) return false;
      const long long m = 2 * q + mate;
      int flag;
      const SamSeq* other = nullptr;
      if (ncomp == 1) {
        if (paired) {
          if (nseq != 2) return false;
          other = &sas[1 - k];
          flag = 1 | 2 | (sa.rev ? 0x10 : 0) | (other->rev ? 0x20 : 0) | (k == 0 ? 0x40 : 0x80);
        } else {
          flag = sa.rev ? 0x10 : 0;
        }
      } else {
        flag = 1 | 8 | (sa.rev ? 0x10 : 0) | (mate == 0 ? 0x40 : 0x80);
      }
      const int len = b.mateLength[m];
      sink.bytesAt(b.names + b.nameOff[m], b.nameOff[m + 1] - b.nameOff[m]);
      sink.compose([&](char* p) { int n = 0; p[n++] = '\t'; n += samPutInt(p + n, flag); p[n++] = '\t'; return n; });
      sink.bytesAt(contigs.names + contigs.off[sa.contig], contigs.off[sa.contig + 1] - contigs.off[sa.contig]);
      sink.compose([&](char* p) { int n = 0; p[n++] = '\t'; n += samPutInt(p + n, (long long)sa.blocks[1] + 1); n += samPutText(p + n, "\t255\t"); return n; });
      samCigar(sa, len, sink);
      if (other) {
        sink.compose([&](char* p) { p[0] = '\t'; return 1; });
        sink.bytesAt(contigs.names + contigs.off[other->contig], contigs.off[other->contig + 1] - contigs.off[other->contig]);
        sink.compose([&](char* p) { int n = 0; p[n++] = '\t'; n += samPutInt(p + n, (long long)other->blocks[1] + 1); p[n++] = '\t'; n += samPutInt(p + n, len); p[n++] = '\t'; return n; });
      } else {
        sink.compose([&](char* p) { int n = samPutText(p, "\t*\t0\t"); n += samPutInt(p + n, len); p[n++] = '\t'; return n; });
      }
      sink.seq(b.codes + b.mateOffset[m], len, sa.rev != 0);
      sink.compose([&](char* p) {
        int n = samPutText(p, "\t*");
        if (ncomp != 1) n += samPutText(p + n, "\tcs:f:0.0");
        else if (paired) { n += samPutText(p + n, "\tcs:f:"); n += samPutDouble(p + n, dbls[0]); }
        n += samPutText(p + n, "\tAS:f:");
        n += samPutDouble(p + n, dbls[3]);
        p[n++] = '\n';
        return n;
      });
      sink.endRecord();
    }
    return true;
  }
};

// The records of query q to the sink.  false: the slice is malformed (xm_result_walk.h, or what SamRecords refuses), and nothing the sink got counts.
template <class Sink>
XM_SAM_WALK bool samWalkQuery(const SamBatch& b, const ResultStreams& st, const SamContigs& contigs, long long q, Sink& sink) {
  SamRecords<Sink> records{b, contigs, q, sink};
  return resultWalkQuery(ResultStreams{st.ints, st.dbls, st.intOff, st.dblOff, contigs.num}, q, records);
}

}  // namespace xm
