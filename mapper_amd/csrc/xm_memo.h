// The run-wide memory of aligned queries (xm_context_set_memo; DESIGN.md "Identical queries"): the other half of the reference's AlignmentCache
// (AlignerWorker.checkCacheAndAlign, AlignerWorker.java:264-291, looks every query up in a cache that spans the run; xm_collapse.h spans one batch).
// Per context (xm_context_set_memo) or per GPU, shared by the contexts attached to it (xm_memory_new), in HBM: one or two GENERATIONS, each an
// open-addressing table of 64-bit fingerprints with one record offset per slot and a byte arena of records bump-allocated from one cursor (layout,
// sizes, table rules and the rules of the generations: xm_memo_plan.h, whose functions the kernels below call).  Per align call, after the batch's collapse:
//   1 xm_memo_lookup_kernel   one wave per representative: the collapse's fingerprint, a linear probe, and on a key match the record's header and bytes
//                             compared with the query across the lanes - in the young generation first, then in the old one.  hit[q] = the record's
//                             offset in the whole arena (which says where it is), -1 = a miss.
//   2 the scan over CollapseListed (xm_collapse.h) with hit[] in its predicate: the representatives that missed, ascending - the first pass's work list
//   3 xm_memo_replay_kernel   before the passes, one wave per representative (a miss leaves at once): room in the call's result arenas from the call's own
//                             cursors, the two slices copied, offsets, lengths and status set to what a read a pass finished has
//   3b xm_memo_promote_kernel the hits of the old generation copied into the young one, when it takes them all (second chance)
//   ... the passes over the misses ...
//   4a xm_memo_measure_kernel (two generations) how many representatives this call aligned and the bytes of their records: the host turns the generations
//                             when the young one does not take them all
//   4 xm_memo_insert_kernel   after the last pass, one wave per representative this call aligned: claim a slot, reserve a record, copy query and slices -
//                             in the young generation
// As in xm_collapse.h, no launch reads what another workgroup of the same launch wrote (the per-XCD L2s are not coherent): only device-scope atomics - the
// compare-and-swap on a key, the arena's cursor, the counters - cross workgroups inside a launch; records and offsets are written in one launch and read in
// later ones only.  Launches of different contexts never touch a memory at the same time: the host holds the memory's mutex from before 1 until 3b has
// completed on the call's stream, and from before 4a until 4 has (xm_capi.hip, struct Memory).
// Invariant: a query is only ever served from a byte-identical query aligned earlier, by a context of the same memory, under bit-identical parameters; the fingerprint decides how
// much is saved, never the output.
#pragma once
#include "xm_collapse.h"
#include "xm_memo_plan.h"

namespace xm {

// One or two generations in one allocation each (xm_memo_plan.h "the memory of a GPU"): generation g's table is keys / offs + g * (mask + 1), its records
// are arena + g * arenaBytes, its state words state + g * 4.  The lookup, the replay and the promotion see the whole memory; the insert is handed the
// young generation alone, as a memory of one generation (generation()).
struct MemoView {
  unsigned long long* keys;   // [generations * (mask + 1)], 0 = empty
  unsigned long long* offs;   // [generations * (mask + 1)], XM_MEMO_DEAD = taken, never matching; else the record's offset in its generation's arena
  unsigned long long mask;    // of one generation's table
  uint8_t* arena;
  unsigned long long arenaBytes;  // of one generation
  unsigned long long* state;  // per generation: [0] slots claimed, [1] the arena's cursor, [2] records stored
  int fingerprintBits;        // XM_MEMO_FINGERPRINT_BITS (64: all of them)
  int generations, young;
  __host__ __device__ MemoView generation(int g) const {
    return MemoView{keys + (unsigned long long)g * (mask + 1), offs + (unsigned long long)g * (mask + 1), mask, arena + (unsigned long long)g * arenaBytes, arenaBytes, state + g * 4, fingerprintBits, 1, 0};
  }
};

__device__ __forceinline__ long long xmWaveItem() { return (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }

// hit[q], fp[q] for the representatives reps[0 .. nReps); totals[0..2] += hits, their ints, their doubles (lanes 0..2: one atomic instruction per wave that hit);
// totals[4..5] += the hits found in the old generation only, the bytes of their records (what a promotion would need in the young one)
__global__ void __launch_bounds__(256) xm_memo_lookup_kernel(BatchView batch, const int64_t* reps, long long nReps, MemoView memo, int64_t* hit, unsigned long long* fp,
                                                             unsigned long long* totals) {
  const long long w = xmWaveItem();
  const int lane = (int)(threadIdx.x & 63u);
  if (w >= nReps) return;
  const long long q = reps[w];
  const unsigned long long h = memoFingerprint(xmQueryFingerprint(batch, q, lane), memo.fingerprintBits);
  MemoHeader hd;
  hd.mateCount = 0; hd.len0 = 0; hd.len1 = 0; hd.intLen = 0; hd.dblLen = 0;
  int generation = memo.young;
  // (the same loads and the same answer in every lane: the wave goes through the generations together)
  const long long at = memoLookupGenerations(memo.keys, memo.offs, memo.mask, memo.arenaBytes, memo.generations, memo.young, h, [&](long long rec) {
    hd = *(const MemoHeader*)(memo.arena + rec);
    const int mc = batch.mateCount[q];
    bool same = hd.mateCount == mc && hd.len0 == batch.mateLength[q * 2] && hd.len1 == (mc > 1 ? batch.mateLength[q * 2 + 1] : 0) && hd.innerBits == xmBits(batch.expectedInner[q]) &&
                hd.deviationBits == xmBits(batch.deviation[q]);
    const uint8_t* stored = memo.arena + rec + memoBytesAt(hd);
    for (int m = 0; m < mc && m < 2 && same; m++) {
      const int len = m == 0 ? hd.len0 : hd.len1;
      const uint8_t* codes = batch.codes + batch.mateOffset[q * 2 + m];
      int differ = 0;
      for (int i = lane; i < len; i += 64) differ |= codes[i] != stored[i];
      same = !__any(differ);
      stored += len;
    }
    return same;
  }, &generation);
  const bool same = at >= 0;
  if (lane == 0) { hit[q] = same ? (int64_t)at : (int64_t)-1; fp[q] = h; }
  if (same && lane < 3) atomicAdd(&totals[lane], lane == 0 ? 1ull : (lane == 1 ? (unsigned long long)hd.intLen : (unsigned long long)hd.dblLen));
  if (same && generation != memo.young && lane < 2) atomicAdd(&totals[4 + lane], lane == 0 ? 1ull : memoRecordBytes(hd));
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

// the hits of this call that the lookup found in the old generation get a second chance: one wave per representative copies the record into the young
// generation - claim the key in the young table, reserve room, copy header, bytes and both slices verbatim (memoPromoteClaim).  The host launches this only when
// the young generation takes all of them (memoPromotes: totals[4..5] of the lookup).  A record whose key is in the young table already (another query with
// the same fingerprint) is dropped.  totals[6] += records copied.  The old records are read only; what is written here is read in later launches only.
__global__ void __launch_bounds__(256) xm_memo_promote_kernel(const int64_t* reps, long long nReps, MemoView memo, const int64_t* hit, const unsigned long long* fp, unsigned long long* totals) {
  const long long w = xmWaveItem();
  const int lane = (int)(threadIdx.x & 63u);
  if (w >= nReps) return;
  const long long q = reps[w];
  const int64_t at = hit[q];
  if (at < 0 || memoGenerationOf((unsigned long long)at, memo.arenaBytes) == memo.young) return;
  const MemoHeader hd = *(const MemoHeader*)(memo.arena + at);
  const unsigned long long bytes = memoRecordBytes(hd);
  const MemoView young = memo.generation(memo.young);
  long long slot = -1;
  unsigned long long to = XM_MEMO_DEAD;
  if (lane == 0) {
    to = memoPromoteClaim(young.keys, young.mask, young.state, young.arenaBytes, fp[q], bytes,
                          [](unsigned long long* a, unsigned long long expected, unsigned long long desired) { return atomicCAS(a, expected, desired); },
                          [](unsigned long long* a, unsigned long long k) { return atomicAdd(a, k); }, &slot);
    if (to != XM_MEMO_DEAD) atomicAdd(&totals[6], 1ull);
  }
  to = (unsigned long long)__shfl((long long)to, 0);
  if (to == XM_MEMO_DEAD) return;
  const unsigned long long* from = (const unsigned long long*)(memo.arena + at);  // (records start on multiples of 8 and are multiples of 8 long)
  unsigned long long* dst = (unsigned long long*)(young.arena + to);
  for (unsigned long long i = (unsigned long long)lane; i < bytes / 8; i += 64) dst[i] = from[i];
  if (lane == 0) young.offs[slot] = to;
}

// list[0 .. n): the representatives this call aligned.  totals[4] += the ones the insert would store (status XM_OK), totals[5] += the exact bytes of their records
// (one thread per item, one pair of atomic instructions per wave): what the host needs to know before the insert whether the young generation takes them all.
__global__ void __launch_bounds__(256) xm_memo_measure_kernel(BatchView batch, const int64_t* list, long long n, OutView out, unsigned long long* totals) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long count = 0, bytes = 0;
  if (i < n) {
    const long long q = list[i];
    if (out.status[q] == XM_OK) {
      const int mc = batch.mateCount[q];
      MemoHeader hd;
      hd.mateCount = mc; hd.len0 = batch.mateLength[q * 2]; hd.len1 = mc > 1 ? batch.mateLength[q * 2 + 1] : 0;
      hd.intLen = out.intLen[q]; hd.dblLen = out.dblLen[q];
      count = 1; bytes = memoRecordBytes(hd);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    count += (unsigned long long)__shfl_xor((long long)count, o);
    bytes += (unsigned long long)__shfl_xor((long long)bytes, o);
  }
  if (lane == 0 && count > 0) { atomicAdd(&totals[4], count); atomicAdd(&totals[5], bytes); }
}

}  // namespace xm
