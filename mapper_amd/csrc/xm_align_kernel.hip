// libxmapper_hip.so: the lane-per-read align kernel in an object of its own, apart from the host side and the C ABI (xm_capi.hip), so that a change
// there neither re-makes nor moves the kernel.
//
// In this file: xm_align_kernel (one read per lane, persistent lanes that draw reads from a counter; the per-read state machine is xm_worker.h), behind
// it the two test kernels that run parts of it alone - they stand in this unit because they must call the same compiled out-of-line functions - and
// the launch functions the host calls (AlignLaunch, TestLocalLaunch, TestBoundLaunch: xm_kernel_common.h).  This is the unit that does not define
// XM_NOINL_LINKAGE: it holds the strong definitions of the out-of-line device functions of xm_seed.h / xm_extend.h / xm_bound.h / xm_wsearch.h /
// xm_worker.h.  The diagnostic device symbols of the kernel (xm_read_times, xm_arrive_prof) are defined here, so their host access is here too.
#include "../../include/xmapper_hip.h"
#include "xm_worker.h"
#include "xm_wsearch.h"
#include "xm_kernel_args.h"
#include "xm_kernel_common.h"
#include <hip/hip_runtime.h>
#include <cstring>

using namespace xm;
namespace {

#ifndef XM_WAVES_PER_SIMD
#define XM_WAVES_PER_SIMD 4  // 128 registers per lane: the path is latency-bound, four waves per SIMD hide more of it than the spills cost
#endif

#ifdef XM_READ_TIMES
// diagnostic builds (-DXM_READ_TIMES, XM_READ_TIMES_FILE=path): shader-clock ticks the last pass spent on every read, written to the file
__device__ unsigned long long* xm_read_times = nullptr;
#endif
// One lane aligns one read at a time (AlignerWorker.align, M/AlignerWorker.java:256-484) and loops until the batch is drained.
__global__ void __launch_bounds__(256, XM_WAVES_PER_SIMD) xm_align_kernel(const LaunchConst* launchConst, BatchView batch, const int64_t* todo, long long nTodo, int scale, int heavyAllowed, int lanesPerWave,
                                                       uint8_t* arenas, unsigned long long arenaBytes, OutView out, unsigned long long* nextItem, DevCounters* counters,
                                                       long long taperUnit, long long firstStride, PNode* waveNodes, HandOver ho, int pairLanes,
                                                       SearchPool searchPool, PassLists lists, int boundFilter) {
  // lanesPerWave < 64 (gapped pass): the extension chain diverges so much that a wave runs its reads nearly one after another, so
  // spreading them over more, partly filled waves shortens the critical path; the idle lanes own no scratch arena
  // index view and parameters: one block in HBM for all lanes (LaunchConst, xm_defs.h) - the lanes hold its address and read it through scalar loads
  const LaunchConstPtr lc = (LaunchConstPtr)launchConst;
  xmSetWaveNodes(waveNodes);
  xmSetPairMode(pairLanes);
  xmSetSearchPool(searchPool);
  xmSetBoundFilter(boundFilter);  // gapped passes of long reads: the rejection filter in front of PathAligner's searches (xm_bound.h)
  xmLoadMergeRule();  // (every thread of the block: it ends with a barrier)
  // pairLanes (gapped pass, lanesPerWave <= 32): a read is run by 2^pairLanes adjacent lanes doing the same work (xm_extend.h, xmSetPairMode: 1 = two lanes,
  // 3 = eight, passes of long reads); `laneInWave` below is the read's slot in the wave, `second` marks the lanes that leave atomics and result writes to the first
  const int physLane = (int)(threadIdx.x & 63u);
  const int groupMask = (1 << pairLanes) - 1;
  const int laneInWave = physLane >> pairLanes;
  const bool second = (physLane & groupMask) != 0;
  if (laneInWave >= lanesPerWave) return;
  unsigned long long lane = ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (unsigned)lanesPerWave + (unsigned)laneInWave;
  uint8_t* arena = arenas + lane * arenaBytes;
  long long myRegion = (long long)lane;  // (mode 1) the pool's first regions are the lanes' initial ones, the cursor starts behind them
  DevCounters local;
  memset(&local, 0, sizeof(local));
  ReadCtx cx;
  // Gapped pass: the list starts with the reads that look expensive.  The first read of every lane is dealt out lane-major (items
  // 0..waves-1 to lane 0 of every wave, the next `waves` items to lane 1, ...), so that every wave gets the same number of them and
  // they all start at once; after that the lanes draw from the counter, which the host has set behind the dealt items.
  bool dealt = firstStride > 0;
  const long long waveIndex = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  while (true) {
    unsigned long long item;
    const long long mine = (long long)laneInWave * firstStride + waveIndex;
    if (dealt && mine < nTodo) {
      dealt = false;
      item = (unsigned long long)mine;
    } else {
      dealt = false;
      {
        // End of the work list (gapped pass): the lanes of a wave run their reads mostly one after the other, so when the list runs dry
        // every wave would still hold lanesPerWave unfinished reads and the launch would end with that long serial tail.  The higher
        // lanes therefore stop taking reads early; the last reads are spread one per wave.
        // (pair mode: the read's first lane decides for both - two separate loads of the counter could differ, and a lane that left alone
        // would leave its partner exchanging values with an inactive lane)
        int leave = 0;
        if (taperUnit > 0 && laneInWave > 0 && !second) {
          long long remaining = nTodo - (long long)__hip_atomic_load(nextItem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          leave = remaining < (long long)laneInWave * taperUnit;
        }
        if (pairLanes) leave = __shfl(leave, physLane & ~groupMask);
        if (leave) break;
      }
      item = 0;
      if (!second) item = atomicAdd(nextItem, 1ull);
      if (pairLanes) item = (unsigned long long)__shfl((long long)item, physLane & ~groupMask);
      if ((long long)item >= nTodo) break;
    }
    int64_t q = todo ? todo[item] : (int64_t)item;
    ReadIn in;
    in.nMates = batch.mateCount[q];
    for (int m = 0; m < 2; m++) {
      in.mate[m] = batch.codes + batch.mateOffset[q * 2 + m];
      in.mateLen[m] = m < in.nMates ? batch.mateLength[q * 2 + m] : 0;
    }
    // single-end Query: expectedInnerDistance 0, deviation 1 (spacing penalty is always 0, T/SamWriter_Test.java:26)
    in.expectedInner = in.nMates > 1 ? batch.expectedInner[q] : 0.0;
    in.deviation = in.nMates > 1 ? batch.deviation[q] : 1.0;
    ReadResult rr;
#ifdef XM_READ_TIMES
    const unsigned long long readT0 = clock64();
#endif
    DevCounters before = local;
    if (ho.mode == 1) {
      uint8_t* region = ho.regions + (unsigned long long)myRegion * ho.regionBytes;
      runReadRetaining(cx, lc, in, scale, region, (size_t)ho.regionBytes, arena, (size_t)arenaBytes, &local, rr, heavyAllowed);
      if (cx.status == XM_ST_NEED_HEAVY && savedReadOf(region, (size_t)ho.regionBytes)->valid) {
        // the read keeps this region; the lane needs a fresh one only if it will take another read (the list counter only grows, so a
        // lane that sees the list drained here finds it drained at its next fetch and leaves)
        const bool drained = (long long)__hip_atomic_load(nextItem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nTodo;
        if (drained) {
          ho.regionOf[q] = (int32_t)myRegion;
        } else {
          long long fresh = (long long)atomicAdd(ho.cursor, 1ull);
          if (fresh < ho.nRegions) { ho.regionOf[q] = (int32_t)myRegion; myRegion = fresh; }  // (pool used up: the read is seeded again by the gapped pass)
        }
      }
    } else if (ho.mode == 2) {
      const int32_t rg = ho.regionOf[q];
      uint8_t* tmp = arena + ho.regionBytes;
      const size_t tmpBytes = (size_t)(arenaBytes - ho.regionBytes);
      if (rg >= 0) runReadResumed(cx, savedReadOf(ho.regions + (unsigned long long)rg * ho.regionBytes, (size_t)ho.regionBytes), lc, scale, tmp, tmpBytes, &local, rr);
      else runReadRetaining(cx, lc, in, ho.seedScale, arena, (size_t)ho.regionBytes, tmp, tmpBytes, &local, rr, 2, scale);
    } else {
      runRead(cx, lc, in, scale, arena, (size_t)arenaBytes, &local, rr, heavyAllowed);
    }
    XM_PAIR_CHECK(0, cx.status);
    XM_PAIR_CHECK(1, ((long long)rr.nComponents << 40) ^ ((long long)rr.single[0] << 20) ^ (long long)rr.empty[0] ^ ((long long)local.pathAlignerNodes << 4));
    int32_t st = cx.status;
#ifdef XM_READ_TIMES
    if (xm_read_times && !second) xm_read_times[q] = clock64() - readT0;
#endif
    if (st != XM_OK) local = before;  // work of a read that is rerun by a later pass is counted there
    if (second) continue;             // (pair mode: the first lane of the read publishes)
    // (a read that found the result arena full is run again too: round 6 - its work used to be counted twice, PathAligner calls and nodes of the first call on a fresh context;
    // pinned by tests/test_gpu_result_stage.py, test_light_pass_overflows_both_arenas: the same batch fresh and warm, equal counters)
    if (publishRead(out, q, rr, cx, local, lists) == XM_ST_OUT_OVERFLOW) local = before;
  }
  if (!second) addCounters(counters, local);
}

// ---------------------------------------------------------------- test kernels: components of the align kernel run alone on given inputs (entries: xm_capi_test.h)
// Test entry (xm_test_local_align): the reference's component-level known-answer tests (PathAligner_Test.java:10-39: PathAligner alone;
// HashBlockAligner_Test.java:10-48: HashBlock_Aligner -> StraightAligner -> PathAligner_Runner) over two given texts, run by the code the align
// kernel runs.  chain 0: one search, in the wave's LDS slot (mode 0), in HBM mode (mode 1) or in the lane-private form (mode 4); chain 1: hashBlockAlign with the searches
// slot-first as in the kernel (mode 0), all in HBM mode (mode 1) or all in the lane-private form of xm_wsearch.h (mode 4).  One lane works; out: found, nb, status, nodes, blocks; penalties.
__global__ void __launch_bounds__(256, XM_WAVES_PER_SIMD) xm_test_local_kernel(int chain, int mode, Params params, const uint8_t* query, int queryLength, const uint8_t* reference, int referenceLength,
                                                            double maxIns, double maxDel, int scale, uint8_t* arena, unsigned long long arenaBytes, PNode* waveNodes, int blockCap,
                                                            int32_t* outInts, double* outDbls) {
  xmSetWaveNodes(waveNodes);
  xmSetPairMode(0);
  xmSetSearchPool(SearchPool{nullptr, 0, 0, 0});
  xmSetBoundFilter(mode >= 8 ? 1 : 0);  // (mode + 8: the search behind the rejection filter of xm_bound.h)
  mode &= 7;
  xmLoadMergeRule();  // (every thread of the block: it ends with a barrier)
  if (threadIdx.x != 0) return;
  DevCounters local;
  memset(&local, 0, sizeof(local));
  Caps caps = makeCaps(scale);
  caps.searchInHbmOnly = mode == 1 ? 1 : (mode == 4 ? 2 : 0);
  Arena tmp;
  tmp.init(arena, (size_t)arenaBytes);
  int32_t status = XM_OK;
  float hint = 0;
  ExtEnv e;
  e.caps = &caps; e.dc = &local; e.status = &status; e.tmp = &tmp;
  e.query.base = query; e.query.len = queryLength; e.query.rc = 0; e.query.id = 0;
  e.reference.base = reference; e.reference.len = referenceLength; e.reference.rc = 0; e.reference.id = 0;
  e.contig = 0;
  e.heavyHint = &hint;
  Matcher* slots = arenaArray<Matcher>(tmp, 3);
  for (int i = 0; i < 3; i++) {
    slots[i].present = arenaArray<uint8_t>(tmp, caps.maxSections);
    slots[i].tables = arenaArray<int16_t>(tmp, caps.matcherEntries);
    slots[i].tableCap = caps.matcherEntries;
    slots[i].maxSections = caps.maxSections;
    slots[i].nSections = 0;
    slots[i].presentMask = 0;
    slots[i].sectionLength = 0;
  }
  e.slotA = &slots[0]; e.slotB = &slots[1]; e.slotT = &slots[2];
  SeqAl out;
  out.blocks = arenaArray<ABlock>(tmp, caps.maxBlocks);
  out.nb = 0; out.contig = 0; out.referenceReversed = 0; out.seqAId = 0; out.totalPenalty = 0; out.alignedPenalty = 0;
  bool found = false;
  if (tmp.overflow) status = XM_ST_OVERFLOW;
  else {
    const Section qs{0, queryLength}, rs{0, referenceLength};
    Analysis an;  // AlignmentAnalysis as the tests construct it: nothing known about the offset, the two extension limits given
    an.matcher = nullptr; an.predictedBestOffset = 0; an.lastCheckedOffset = 0; an.confidentAboutBestOffset = false;
    an.maxInsertionExtensionPenalty = maxIns; an.maxDeletionExtensionPenalty = maxDel;
    if (chain == 0) found = pathAlign(e, qs, rs, params, an, out);
    else found = hashBlockAlign(e, qs, rs, params, an, out, e.slotB, NextStraight3());
  }
  outInts[0] = found && status == XM_OK ? 1 : 0; outInts[1] = found ? out.nb : 0; outInts[2] = status; outInts[3] = (int32_t)local.pathAlignerNodes;
  outInts[4 + 4 * blockCap] = (int32_t)local.boundChecks; outInts[5 + 4 * blockCap] = (int32_t)local.boundRejects; outInts[6 + 4 * blockCap] = (int32_t)local.boundCells;  // (behind the blocks)
  if (found) {
    for (int i = 0; i < out.nb && i < blockCap; i++) { outInts[4 + 4 * i] = out.blocks[i].startA; outInts[5 + 4 * i] = out.blocks[i].startB; outInts[6 + 4 * i] = out.blocks[i].lenA; outInts[7 + 4 * i] = out.blocks[i].lenB; }
    outDbls[0] = out.totalPenalty; outDbls[1] = out.alignedPenalty;
  }
}

// Test entry (xm_test_bound): the rejection filter of xm_bound.h alone, on one problem - a section of a query against a window of a reference - as a lane of a
// long-read chain runs it (lane 0 of a wave, its region of the wave's slot; pair = 1: lanes 0 and 1 together, 3: lanes 0 .. 7).  out: taken, rejected, cells.
__global__ void __launch_bounds__(256, XM_WAVES_PER_SIMD) xm_test_bound_kernel(Params params, const uint8_t* query, int queryLength, int queryRc, int startA, int endA, const uint8_t* reference, int referenceLength,
                                                            int startB, int endB, int predictedBestOffset, int pair, uint8_t* arena, unsigned long long arenaBytes, int64_t* out) {
  xmSetWaveNodes(nullptr);
  xmSetPairMode(pair);
  xmSetSearchPool(SearchPool{nullptr, 0, 0, 0});
  xmSetBoundFilter(3);
  xmLoadMergeRule();  // (every thread of the block: it ends with a barrier)
  if (threadIdx.x >= (1u << pair)) return;
  const BoundProblem bp = boundTestProblem(params, query, queryLength, queryRc, startA, endA, reference, referenceLength, startB, endB, predictedBestOffset);
  bool taken = false;
  unsigned long long cells = 0;
  Arena tmp;
  tmp.init(arena, (size_t)arenaBytes);  // (the two lanes of a pair keep the same band in the same memory, as they do in the passes: same values twice)
  const bool rejected = boundRejects(bp, pair, tmp, taken, cells);
  if (threadIdx.x == 0) { out[0] = taken ? 1 : 0; out[1] = rejected ? 1 : 0; out[2] = (int64_t)cells; }
}

}  // namespace

namespace xm {

int xmAlignLaunch(const AlignLaunch& a, void* stream) {
  hipLaunchKernelGGL(xm_align_kernel, dim3(a.grid), dim3(a.block), 0, (hipStream_t)stream, a.launchConst, a.batch, a.todo, a.nTodo, a.scale, a.heavyAllowed, a.lanesPerWave,
                     a.arenas, a.arenaBytes, a.out, a.nextItem, a.counters, a.taperUnit, a.firstStride, a.waveNodes, a.ho, a.pairLanes, a.searchPool, a.lists, a.boundFilter);
  return (int)hipGetLastError();
}
int xmTestLocalLaunch(const TestLocalLaunch& t, void* stream) {
  hipLaunchKernelGGL(xm_test_local_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t.chain, t.mode, t.params, t.query, t.queryLength, t.reference, t.referenceLength,
                     t.maxIns, t.maxDel, t.scale, t.arena, t.arenaBytes, t.waveNodes, t.blockCap, t.outInts, t.outDbls);
  return (int)hipGetLastError();
}
int xmTestBoundLaunch(const TestBoundLaunch& t, void* stream) {
  hipLaunchKernelGGL(xm_test_bound_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t.params, t.query, t.queryLength, t.queryRc, t.startA, t.endA, t.reference, t.referenceLength,
                     t.startB, t.endB, t.predictedBestOffset, t.pair, t.arena, t.arenaBytes, t.out);
  return (int)hipGetLastError();
}
#ifdef XM_READ_TIMES
int xmSetReadTimes(unsigned long long* perRead) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(xm_read_times), &perRead, sizeof(perRead)); }
#endif
#ifdef XM_PROFILE
int xmTakeArriveProf(unsigned long long* out16) {
  const unsigned long long zero[16] = {0};
  const hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(xm_arrive_prof), sizeof(zero));
  return (int)(e != hipSuccess ? e : hipMemcpyToSymbol(HIP_SYMBOL(xm_arrive_prof), zero, sizeof(zero)));
}
#endif

}  // namespace xm
