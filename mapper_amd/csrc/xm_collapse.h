// Collapsing of identical queries within a batch (xm_context_set_collapse; DESIGN.md "Identical queries").  The reference aligns a query it has
// already seen only once: AlignerWorker.checkCacheAndAlign (AlignerWorker.java:264-291) looks it up in the run's AlignmentCache and, on a hit,
// binds the cached alignments to the new query (:273-275).  Here, per resident batch, on the device and in separate launches (no phase reads what
// another workgroup of the same launch wrote: the per-XCD L2s are not coherent):
//   1 xm_collapse_fingerprint_kernel  one wave per query: a 64-bit fingerprint over everything the alignment of the query reads (mate count, each
//                                     mate's length and bytes in order, the bit patterns of expected_inner and deviation), inserted into an
//                                     open-addressing table (device-scope CAS claims the key, atomicMin keeps the lowest query index)
//   2 xm_collapse_verify_kernel       one wave per query: a query whose slot holds a lower index is compared with that query byte for byte; any
//                                     difference (a fingerprint collision) makes it its own representative.  repOf[q] = the query q is served from.
//   3 the scan of xm_scan.h over CollapseListed
//                                     the representatives in ascending query order: the first pass's work list (with the run-wide memory, xm_memo.h, a
//                                     second time over the representatives it did not hold: the predicate is an argument)
//   4 xm_collapse_fanout_kernel       after the last pass: every copy's slice (offsets and lengths in the result arena) is its representative's
// Invariant: a query is only ever served from a byte-identical query of the same batch; the fingerprint decides how much is saved, never the output.
#pragma once
#include "xm_kernel_args.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace xm {

__device__ __forceinline__ unsigned long long xmCollapseMix(unsigned long long z) {  // SplitMix64's finaliser
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long xmBits(double x) { return (unsigned long long)__double_as_longlong(x); }

// The fingerprint of query q, computed by one wave (lane = 0..63) and returned in every lane: 64 bits over everything the alignment of the query reads.  Never 0.
// (xm_collapse_fingerprint_kernel and the run-wide memory's xm_memo_lookup_kernel, xm_memo.h, both key their tables with it.)
__device__ __forceinline__ unsigned long long xmQueryFingerprint(const BatchView& batch, long long q, int lane) {
  const int mc = batch.mateCount[q];
  // the sum over the bases of mix(mate, position, code): order-sensitive (the position is in every term), reduced across the lanes
  unsigned long long acc = 0;
  int lens[2] = {0, 0};
  for (int m = 0; m < mc && m < 2; m++) {
    const int len = batch.mateLength[q * 2 + m];
    lens[m] = len;
    const uint8_t* codes = batch.codes + batch.mateOffset[q * 2 + m];
    for (int i = lane; i < len; i += 64)
      acc += xmCollapseMix(((((unsigned long long)m << 16) | (unsigned)i) << 8 | codes[i]) + 0x9E3779B97F4A7C15ull);
  }
  for (int d = 32; d > 0; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, d);
  unsigned long long h = xmCollapseMix(acc ^ xmCollapseMix((unsigned long long)mc | ((unsigned long long)lens[0] << 2) | ((unsigned long long)lens[1] << 33)));
  h = xmCollapseMix(h ^ xmBits(batch.expectedInner[q]));
  h = xmCollapseMix(h ^ xmCollapseMix(xmBits(batch.deviation[q]) + 0xD1B54A32D192ED03ull));
  return h == 0 ? 1 : h;  // (0 marks an empty slot)
}

// table: keys[cap] (0 = empty), reps[cap] (lowest query index of the slot; ~0 = none), cap a power of two >= 2 nq.  repOf[q] <- q's slot.
__global__ void __launch_bounds__(256) xm_collapse_fingerprint_kernel(BatchView batch, unsigned long long* keys, unsigned long long* reps, unsigned long long mask, int64_t* repOf) {
  const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63u);
  if (q >= batch.nq) return;
  const unsigned long long h = xmQueryFingerprint(batch, q, lane);
  if (lane != 0) return;
  unsigned long long slot = h & mask;
  while (true) {  // (at most half the slots are taken: the probe ends)
    const unsigned long long was = atomicCAS(&keys[slot], 0ull, h);
    if (was == 0 || was == h) break;
    slot = (slot + 1) & mask;
  }
  atomicMin(&reps[slot], (unsigned long long)q);
  repOf[q] = (int64_t)slot;
}

// repOf[q]: q's slot (fingerprint kernel) -> the query q is served from (q itself for a representative)
__global__ void __launch_bounds__(256) xm_collapse_verify_kernel(BatchView batch, const unsigned long long* reps, int64_t* repOf) {
  const long long q = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63u);
  if (q >= batch.nq) return;
  const long long r = (long long)reps[repOf[q]];
  bool same = r < q;
  const int mc = batch.mateCount[q];
  if (same) same = batch.mateCount[r] == mc && xmBits(batch.expectedInner[r]) == xmBits(batch.expectedInner[q]) && xmBits(batch.deviation[r]) == xmBits(batch.deviation[q]);
  for (int m = 0; m < mc && same; m++) {
    const int len = batch.mateLength[q * 2 + m];
    if (batch.mateLength[r * 2 + m] != len) { same = false; break; }
    const int64_t oq = batch.mateOffset[q * 2 + m], orr = batch.mateOffset[r * 2 + m];
    if (oq == orr) continue;  // (mates that point at the same bytes)
    int differ = 0;
    for (int i = lane; i < len; i += 64) differ |= batch.codes[oq + i] != batch.codes[orr + i];
    same = !__any(differ);
  }
  if (lane == 0) repOf[q] = same ? (int64_t)r : (int64_t)q;
}

// The work list's predicate: q is a representative and, where the run-wide memory looked the representatives up (xm_memo.h: hit[q] = the record's offset, -1 =
// a miss; null without the memory), it missed.
__device__ __forceinline__ bool xmListed(const int64_t* repOf, const int64_t* hit, long long q) { return repOf[q] == q && (hit == nullptr || hit[q] < 0); }

// The work list as a scan (xm_scan.h) of the predicate: list[0 .. total[0]) = the listed queries in ascending query order, total[0] = how many
struct CollapseListed {
  static constexpr int N = 1;
  long long nq;
  const int64_t* repOf; const int64_t* hit;
  int64_t* list; unsigned long long* total;
  __device__ long long count() const { return nq; }
  __device__ void lens(long long q, long long v[1]) const { v[0] = xmListed(repOf, hit, q) ? 1 : 0; }
  __device__ void put(long long q, const long long at[1]) const { if (xmListed(repOf, hit, q)) list[at[0]] = q; }
  __device__ void totals(const long long t[1]) const { total[0] = (unsigned long long)t[0]; }
};

// every copy's slice is its representative's (the representatives were written by the passes, in earlier launches; no copy is a representative)
__global__ void __launch_bounds__(256) xm_collapse_fanout_kernel(long long nq, const int64_t* repOf, int64_t* intOff, int64_t* dblOff, int32_t* intLen, int32_t* dblLen) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int64_t r = repOf[q];
  if (r == q) return;
  intOff[q] = intOff[r]; dblOff[q] = dblOff[r]; intLen[q] = intLen[r]; dblLen[q] = dblLen[r];
}

}  // namespace xm
