// The queries of a batch counted per combination of contigs on the GPU, from the result streams where an align call left them (included once,
// by xm_capi.hip): the kernels over the plain rules of xm_refs_rules.h.  A lane per query, separate launches, and no launch reads with plain loads what
// another workgroup of the same launch stored (the XCDs' L2s are not coherent within a launch): inside a launch only device-scope atomics are shared.
//   claim     every lane walks its slice.  A malformed slice leaves the lowest such query in the control word.  An aligned query of at most XM_REFS_INLINE
//             contigs claims the slot of its set's fingerprint in an open-addressing table (CAS on keys[], linear probing past other fingerprints) and
//             leaves the lowest query of the slot in reps[] - once per distinct fingerprint of the wavefront, not per lane; slotOf[q] = the slot, -1 for a
//             query without alignment, -2 for a wide one (leftLen[q] = nSeq)
//   verify    a lane with a slot compares its set with that of the slot's representative (the representative's slice walked again): equal - it is counted
//             on the slot; different - a fingerprint collision: slotOf[q] = -2, leftLen[q] = nSeq, the host counts it.  The count is one atomic add per
//             distinct slot per wavefront, not per lane: a reference of one contig sends every aligned query of a batch to one address.
//   offsets   exclusive sums in query order of isRep, leftLen and leftFlag: one scan of xm_scan.h over the three int32 arrays
//   gather    a representative walks again and writes its record {count, n, ids} at records[off[q]]; a left-over query writes its nSeq contigs, repeats and
//             stream order kept, at left[loff[q] .. loff[q + 1]) and where they start at leftStart[lqoff[q]].  No lane stores outside its own range or behind
//             a buffer's end, whatever the second walk yields.
// The fingerprint decides how much the host is left with, never the output: a set is only ever counted on a slot whose representative has the same set.
#pragma once
#include "xm_refs_rules.h"
#include "../../include/xmapper_hip.h"
#include <hip/hip_runtime.h>

namespace {

constexpr unsigned long long XM_REFS_NO_REP = ~0ull;
constexpr int32_t XM_REFS_UNALIGNED = -1, XM_REFS_LEFT = -2;  // slotOf[q] of a query that has no slot

// ctl[0]: the lowest query with a malformed slice (xm::XM_NO_QUERY: none); ctl[1]: aligned queries
constexpr int XM_REFS_CTL_WORDS = 2;

// keys[cap] (0 = empty), reps[cap] (the lowest query of the slot; XM_REFS_NO_REP = none), counts[cap]; cap a power of two >= 2 nq, mask = cap - 1
struct RefsTable { unsigned long long* keys; unsigned long long* reps; unsigned long long* counts; unsigned long long mask; };

__global__ void __launch_bounds__(256) xm_refs_claim_kernel(xm::ResultStreams st, long long nq, int bits, RefsTable table, int32_t* slotOf, int32_t* leftLen, int32_t* leftFlag,
                                                            unsigned long long* ctl) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  xm::RefSet s;
  unsigned long long h = 0;
  if (q < nq) {  // (lanes behind the last query stay for the ballots and add nothing)
    if (!xm::refsWalkQuery(st, q, s)) { atomicMin(&ctl[0], (unsigned long long)q); s = xm::RefSet(); }
    if (s.aligned && !s.wide) h = xm::refsFingerprint(s.ids, s.n, bits);  // (never 0)
  }
  // One claim per distinct fingerprint of the wavefront, like the tally: the lowest live lane - the lowest query of its fingerprint here, since queries
  // ascend with the lanes - probes, claims and leaves its query in reps[], and the lanes with the same fingerprint take its slot.
  int32_t slot = s.aligned ? XM_REFS_LEFT : XM_REFS_UNALIGNED;
  unsigned long long live = __ballot(h != 0);
  while (live) {
    const int leader = __ffsll((long long)live) - 1;
    const unsigned long long mine = __shfl(h, leader, 64);
    unsigned long long at = 0;
    if (lane == leader) {
      at = mine & table.mask;
      while (true) {  // (at most half the slots are taken: the probe ends)
        const unsigned long long was = atomicCAS(&table.keys[at], 0ull, mine);
        if (was == 0 || was == mine) break;
        at = (at + 1) & table.mask;
      }
      atomicMin(&table.reps[at], (unsigned long long)q);
    }
    at = __shfl(at, leader, 64);
    if (h == mine) slot = (int32_t)at;  // (cap <= 2^31: refsRun refuses more queries than that allows)
    live &= ~__ballot(h == mine);
  }
  if (q < nq) {
    slotOf[q] = slot;
    leftLen[q] = slot == XM_REFS_LEFT ? s.nSeq : 0;
    leftFlag[q] = slot == XM_REFS_LEFT ? 1 : 0;
  }
  const unsigned long long all = __ballot(s.aligned);
  if (lane == 0 && all) atomicAdd(&ctl[1], (unsigned long long)__popcll(all));
}

__global__ void __launch_bounds__(256) xm_refs_verify_kernel(xm::ResultStreams st, long long nq, RefsTable table, int32_t* slotOf, int32_t* leftLen, int32_t* leftFlag, int32_t* isRep) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  bool counted = false;
  int32_t slot = XM_REFS_UNALIGNED;
  if (q < nq) {
    slot = slotOf[q];
    bool rep = false;
    if (slot >= 0) {
      const unsigned long long r = table.reps[slot];  // (stored by the claim launch)
      rep = r == (unsigned long long)q;
      counted = rep;
      if (!rep) {
        xm::RefSet mine, theirs;
        const bool ok = r < (unsigned long long)nq && xm::refsWalkQuery(st, q, mine) && xm::refsWalkQuery(st, (long long)r, theirs);
        counted = ok && mine.aligned && theirs.aligned && xm::refsSame(mine, theirs);
        if (!counted) {  // a fingerprint collision: the host counts this one
          slotOf[q] = XM_REFS_LEFT;
          leftLen[q] = ok ? mine.nSeq : 0;
          leftFlag[q] = ok ? 1 : 0;
        }
      }
    }
    isRep[q] = rep ? 1 : 0;
  }
  // one add per distinct slot of the wavefront: the lanes of the lowest live lane's slot are counted by that lane, until no lane is live
  unsigned long long live = __ballot(counted);
  while (live) {
    const int leader = __ffsll((long long)live) - 1;
    const int32_t s = __shfl(slot, leader, 64);
    const unsigned long long same = __ballot(counted && slot == s);
    if (lane == leader) atomicAdd(&table.counts[s], (unsigned long long)__popcll(same));
    live &= ~same;
  }
}

// the record of one combination as the host gets it (xm_refs_record, include/xmapper_hip.h)
struct RefsRecord { int64_t count; int32_t n; int32_t ids[xm::XM_REFS_INLINE]; int32_t reserved; };
static_assert(sizeof(RefsRecord) == sizeof(xm_refs_record), "RefsRecord is xm_refs_record");

// the sink of the gather: the contig of sequence alignment k to out[lo + k], if that is inside the query's own range and the buffer
struct RefsContigStore {
  int32_t* out;
  long long lo, hi, cap;
  __device__ void contig(long long k, int32_t c) {
    const long long at = lo + k;
    if (k >= 0 && at < hi && at < cap) out[at] = c;
  }
};

__global__ void __launch_bounds__(256) xm_refs_gather_kernel(xm::ResultStreams st, long long nq, RefsTable table, const int32_t* slotOf, const int64_t* off, const int64_t* loff,
                                                             const int64_t* lqoff, RefsRecord* records, long long recordCap, int32_t* left, long long leftCap, int64_t* leftStart,
                                                             long long leftStartCap) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const long long at = off[q];
  const int32_t slot = slotOf[q];
  if (records && off[q + 1] > at && at >= 0 && at < recordCap && slot >= 0 && (unsigned long long)slot <= table.mask) {
    xm::RefSet s;
    if (xm::refsWalkQuery(st, q, s) && !s.wide) {
      RefsRecord r;
      r.count = (int64_t)table.counts[slot];  // (added up by the verify launch)
      r.n = s.n;
      for (int i = 0; i < xm::XM_REFS_INLINE; i++) r.ids[i] = i < s.n ? s.ids[i] : 0;
      r.reserved = 0;
      records[at] = r;
    }
  }
  const long long lo = loff[q], hi = loff[q + 1];
  if (left && hi > lo && lo >= 0) {
    RefsContigStore sink{left, lo, hi, leftCap};
    xm::RefSet s;
    (void)xm::refsWalkQuery(st, q, s, sink);
  }
  if (leftStart) {
    const long long k = lqoff[q];
    if (lqoff[q + 1] > k && k >= 0 && k < leftStartCap) leftStart[k] = lo;
  }
}

}  // namespace
