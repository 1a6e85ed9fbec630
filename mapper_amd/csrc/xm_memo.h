// The run-wide memory of aligned queries (xm_context_set_memo; DESIGN.md "Identical queries"): the other half of the reference's AlignmentCache
// (AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291, looks every query up in a cache that spans the run; xm_collapse.h spans one batch).
// Per context, in HBM: an open-addressing table of 64-bit fingerprints with one record offset per slot, and a byte arena of records bump-allocated from
// one cursor (layout, sizes and table rules: xm_memo_plan.h, whose functions the kernels below call).  Per align call, after the batch's collapse:
//   1 xm_memo_lookup_kernel   one wave per representative: the collapse's fingerprint, a linear probe, and on a key match the record's header and bytes
//                             compared with the query across the lanes.  hit[q] = the record's offset, -1 = a miss.
//   2 xm_collapse_count / scan / compact_kernel with hit[] as their predicate: the representatives that missed, ascending - the first pass's work list
//   3 xm_memo_replay_kernel   before the passes, one wave per representative (a miss leaves at once): room in the call's result arenas from the call's own
//                             cursors, the two slices copied, offsets, lengths and status set to what a read a pass finished has
//   ... the passes over the misses ...
//   4 xm_memo_insert_kernel   after the last pass, one wave per representative this call aligned: claim a slot, reserve a record, copy query and slices
// As in xm_collapse.h, no launch reads what another workgroup of the same launch wrote (the per-XCD L2s are not coherent): only device-scope atomics - the
// compare-and-swap on a key, the arena's cursor, the counters - cross workgroups inside a launch; records and offsets are written in one launch and read in
// later ones only.
// Invariant: a query is only ever served from a byte-identical query this context aligned earlier under bit-identical parameters; the fingerprint decides how
// much is saved, never the output.
#pragma once
#include "xm_collapse.h"
#include "xm_memo_plan.h"

namespace xm {

struct MemoView {
  unsigned long long* keys;   // [mask + 1], 0 = empty
  unsigned long long* offs;   // [mask + 1], XM_MEMO_DEAD = taken, never matching
  unsigned long long mask;
  uint8_t* arena;
  unsigned long long arenaBytes;
  unsigned long long* state;  // [0] slots claimed, [1] the arena's cursor, [2] records stored
  int fingerprintBits;        // XM_MEMO_FINGERPRINT_BITS (64: all of them)
};

__device__ __forceinline__ long long xmWaveItem() { return (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }

// hit[q], fp[q] for the representatives reps[0 .. nReps); totals[0..2] += hits, their ints, their doubles (lanes 0..2: one atomic instruction per wave that hit)
__global__ void __launch_bounds__(256) xm_memo_lookup_kernel(BatchView batch, const int64_t* reps, long long nReps, MemoView memo, int64_t* hit, unsigned long long* fp,
                                                             unsigned long long* totals) {
  const long long w = xmWaveItem();
  const int lane = (int)(threadIdx.x & 63u);
  if (w >= nReps) return;
  const long long q = reps[w];
  const unsigned long long h = memoFingerprint(xmQueryFingerprint(batch, q, lane), memo.fingerprintBits);
  const long long at = memoSlotRecord(memo.offs, memoProbe(memo.keys, memo.mask, h));  // (the same loads in every lane)
  bool same = at >= 0;
  MemoHeader hd;
  hd.intLen = 0; hd.dblLen = 0;
  if (same) {
    hd = *(const MemoHeader*)(memo.arena + at);
    const int mc = batch.mateCount[q];
    same = hd.mateCount == mc && hd.len0 == batch.mateLength[q * 2] && hd.len1 == (mc > 1 ? batch.mateLength[q * 2 + 1] : 0) && hd.innerBits == xmBits(batch.expectedInner[q]) &&
           hd.deviationBits == xmBits(batch.deviation[q]);
    const uint8_t* stored = memo.arena + at + memoBytesAt(hd);
    for (int m = 0; m < mc && m < 2 && same; m++) {
      const int len = m == 0 ? hd.len0 : hd.len1;
      const uint8_t* codes = batch.codes + batch.mateOffset[q * 2 + m];
      int differ = 0;
      for (int i = lane; i < len; i += 64) differ |= codes[i] != stored[i];
      same = !__any(differ);
      stored += len;
    }
  }
  if (lane == 0) { hit[q] = same ? (int64_t)at : (int64_t)-1; fp[q] = h; }
  if (same && lane < 3) atomicAdd(&totals[lane], lane == 0 ? 1ull : (lane == 1 ? (unsigned long long)hd.intLen : (unsigned long long)hd.dblLen));
}

// every representative that hit gets its record's slices in the call's result arenas.  The host sized the arenas for the hits' totals on top of what the passes
// are given, so the room is there; a slice that would not fit is not written and counted in totals[3] (the host fails the call).
__global__ void __launch_bounds__(256) xm_memo_replay_kernel(const int64_t* reps, long long nReps, MemoView memo, const int64_t* hit, OutView out, unsigned long long* totals) {
  const long long w = xmWaveItem();
  const int lane = (int)(threadIdx.x & 63u);
  if (w >= nReps) return;
  const long long q = reps[w];
  const int64_t at = hit[q];
  if (at < 0) return;
  const MemoHeader hd = *(const MemoHeader*)(memo.arena + at);
  unsigned long long io = 0, dofs = 0;
  if (lane == 0) {
    io = atomicAdd(&out.cursor[0], (unsigned long long)hd.intLen);
    dofs = atomicAdd(&out.cursor[1], (unsigned long long)hd.dblLen);
  }
  io = (unsigned long long)__shfl((long long)io, 0);
  dofs = (unsigned long long)__shfl((long long)dofs, 0);
  if (io + (unsigned long long)hd.intLen > out.intCap || dofs + (unsigned long long)hd.dblLen > out.dblCap) {
    if (lane == 0) atomicAdd(&totals[3], 1ull);
    return;
  }
  const int32_t* ints = (const int32_t*)(memo.arena + at + memoIntsAt(hd));
  const double* dbls = (const double*)(memo.arena + at + memoDblsAt(hd));
  for (int i = lane; i < hd.intLen; i += 64) out.ints[io + i] = ints[i];
  for (int i = lane; i < hd.dblLen; i += 64) out.dbls[dofs + i] = dbls[i];
  if (lane == 0) {
    out.intOff[q] = (int64_t)io; out.dblOff[q] = (int64_t)dofs; out.intLen[q] = hd.intLen; out.dblLen[q] = hd.dblLen;
    out.status[q] = XM_OK;
  }
}

// list[0 .. n): representatives this call aligned (every one finished: the last pass has succeeded), fp[q] their fingerprints from the lookup.  n is at most the
// table's room (memoRoom): a launch never takes the table beyond half full.
__global__ void __launch_bounds__(256) xm_memo_insert_kernel(BatchView batch, const int64_t* list, long long n, MemoView memo, const unsigned long long* fp, OutView out) {
  const long long w = xmWaveItem();
  const int lane = (int)(threadIdx.x & 63u);
  if (w >= n) return;
  const long long q = list[w];
  if (out.status[q] != XM_OK) return;
  const int mc = batch.mateCount[q];
  MemoHeader hd;
  hd.mateCount = mc; hd.len0 = batch.mateLength[q * 2]; hd.len1 = mc > 1 ? batch.mateLength[q * 2 + 1] : 0;
  hd.intLen = out.intLen[q]; hd.dblLen = out.dblLen[q]; hd.reserved = 0;
  hd.innerBits = xmBits(batch.expectedInner[q]); hd.deviationBits = xmBits(batch.deviation[q]);
  long long slot = -1;
  unsigned long long at = XM_MEMO_DEAD;
  if (lane == 0) {
    slot = memoClaim(memo.keys, memo.mask, fp[q], [](unsigned long long* a, unsigned long long expected, unsigned long long desired) { return atomicCAS(a, expected, desired); });
    if (slot >= 0) {
      atomicAdd(&memo.state[0], 1ull);
      at = memoReserve(&memo.state[1], memo.arenaBytes, memoRecordBytes(hd), [](unsigned long long* a, unsigned long long k) { return atomicAdd(a, k); });
      if (at != XM_MEMO_DEAD) atomicAdd(&memo.state[2], 1ull);
    }
  }
  at = (unsigned long long)__shfl((long long)at, 0);
  if (at == XM_MEMO_DEAD) return;  // its own key was there already (dropped), or no room in the arena (the slot stays dead)
  uint8_t* rec = memo.arena + at;
  uint8_t* stored = rec + memoBytesAt(hd);
  for (int m = 0; m < mc && m < 2; m++) {
    const int len = m == 0 ? hd.len0 : hd.len1;
    const uint8_t* codes = batch.codes + batch.mateOffset[q * 2 + m];
    for (int i = lane; i < len; i += 64) stored[i] = codes[i];
    stored += len;
  }
  int32_t* ints = (int32_t*)(rec + memoIntsAt(hd));
  double* dbls = (double*)(rec + memoDblsAt(hd));
  const int32_t* fromI = out.ints + out.intOff[q];
  const double* fromD = out.dbls + out.dblOff[q];
  for (int i = lane; i < hd.intLen; i += 64) ints[i] = fromI[i];
  for (int i = lane; i < hd.dblLen; i += 64) dbls[i] = fromD[i];
  if (lane == 0) {
    *(MemoHeader*)rec = hd;
    memo.offs[slot] = at;
  }
}

}  // namespace xm
