// libxmapper_hip.so: the host side of the align call and the C ABI of include/xmapper_hip.h, one translation unit.
//
// In this file, in this order: the two small kernels of its own (the wave form's work lists, the bucket lines); the tables of a reference on the host
// and in HBM (HostShare, DeviceTables); the owners of a context's device buffers - DeviceBatch (the resident and the staged batch), PassBuffers (work
// lists, control words, counters and scratch of the lane-per-read passes), DeviceConfTable (the confidence table and its copy in HBM), WaveFormBuffers,
// CollapseBuffers, MemoCallBuffers - and the context (xm_index) that holds one of each beside its stream and its ResultStage; the steps of an align call
// (AlignCall ... finishStreams), which launch what xm_pass_plan.h plans - reads a pass could not finish are run again by a later pass on the GPU, never
// on the CPU; the C entries for indexes, contexts, batches and alignment (a first context is opened by openFirstContext, whichever entry asks).
// Beside it, included once each: xm_device_rt.h (error checking, DevBuf, the pinned result pool), xm_scan.h (the exclusive prefix sums in item order that
// every output stage below takes: three kernels over a stage's Items, and the block-level sum and scan), xm_result_stage.h (ResultStage: the result arenas,
// the gather kernel, the canonical streams; throwFailedQuery), xm_conf_table.h (the host's confidence table), xm_capi_probe.h (seed-probe and
// random-gather measurements), xm_capi_pileup.h (the pile-up), xm_capi_test.h (test-only entries), xm_capi_fastq.h (a batch staged from FASTQ text: the kernels of xm_fastq.h),
// xm_capi_fasta.h (the same from FASTA text of any number of lines a record: the kernels of xm_fasta.h),
// xm_capi_sam.h (SAM records formatted from the resident results: the kernels of xm_sam.h), xm_capi_summary.h (the statistics, the penalties and the unaligned
// queries of the resident results: the kernels of xm_summary.h), xm_capi_refs.h (the queries of the resident results counted per combination of contigs: the
// kernels of xm_refs.h), xm_capi_unaligned.h (the unaligned-query file's text made from the resident batch and results: the kernels of xm_unaligned.h; and
// the switch that keeps a batch staged from text in HBM).
// The big kernels are objects of their own, reached through launch functions: the lane-per-read align kernel is xm_align_kernel.hip (xmAlignLaunch,
// xm_kernel_common.h), the wave-per-read kernels are xm_wave_kernel.hip (xmWaveLaunch, xm_kernel_args.h), the index build on the device is
// xm_index_device.hip.  This unit uses the host-side pieces of the shared headers only (makeCaps, searchPoolBytes, the pass planner's sizes):
// nothing of the per-read state machine is compiled for the device from here.
#define XM_NOINL_LINKAGE inline  // the out-of-line functions of the shared headers are defined (strongly) by xm_align_kernel.hip
#include "../../include/xmapper_hip.h"
#include "xm_worker.h"
#include "xm_wsearch.h"
#include "xm_index_host.h"
#include "xm_kernel_args.h"
#include "xm_kernel_common.h"
#include "xm_pass_plan.h"
#include "xm_collapse.h"
#include "xm_fastq.h"
#include "xm_fasta.h"
#include "xm_sam.h"
#include "xm_summary.h"
#include "xm_unaligned.h"
#include "xm_refs.h"
#include "xm_memo.h"
#include "xm_conf_table.h"
#include "xm_device_rt.h"
#include "xm_scan.h"
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <mutex>
#include <shared_mutex>
#include <memory>
#include <atomic>
#include <array>
#include <type_traits>
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <cstdio>

namespace xm { bool deviceHashLengths(HostIndex& h, int minLen, int maxLen, int device, const BuildKnobs& knobs); }  // xm_index_device.hip
using namespace xm;
#include "xm_result_stage.h"

namespace {

// ---------------------------------------------------------------- pass bookkeeping on the device (PassCtl, PassLists: xm_kernel_common.h)
// after a pass of the wave-per-read form (xm_wave_kernel.hip): reads for the next tier, reads with a waiting search request, reads left
// to the lane-per-read passes
struct WaveCtl { unsigned long long nNext, nSearch, nFallback, errQuery; };
__global__ void __launch_bounds__(256) xm_wave_classify_kernel(const int64_t* todo, long long nTodo, const int32_t* status, int64_t* listNext, int32_t* slotOfOut, int64_t* listSearch,
                                                               int64_t* listFallback, WaveCtl* ctl) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nTodo) return;
  const int64_t q = todo ? todo[i] : (int64_t)i;
  const int32_t st = status[q] & 0xFF;
  if (st == XM_OK) return;
  if (st == XM_ST_WAVE_GAPPED && listNext) {
    const unsigned long long pos = atomicAdd(&ctl->nNext, 1ull);
    listNext[pos] = q;
    if (slotOfOut) slotOfOut[q] = (int32_t)pos;  // the read's memo (it keeps it through the later tiers)
  } else if (st == XM_ST_WAVE_SEARCH && listSearch) listSearch[atomicAdd(&ctl->nSearch, 1ull)] = q;
  else if (st == XM_ST_WAVE_FALLBACK || st == XM_ST_WAVE_GAPPED || st == XM_ST_WAVE_SEARCH) listFallback[atomicAdd(&ctl->nFallback, 1ull)] = q;
  else atomicMin(&ctl->errQuery, (unsigned long long)q);
}

// Bucket lines of one table from its CSR form (IndexView::lines32 / lines64): one lane per bucket.
template <typename W, typename P>
__global__ void __launch_bounds__(256) xm_lines_kernel(Table t, const uint32_t* bucketOff, const P* positions, W* lines) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= t.capacity) return;
  const uint32_t* off = bucketOff + t.offBase + k;
  W line[8];
  xmFillLine(line, off[0], off[1], positions + t.posBase);
  W* dst = lines + (t.offBase + k) * 8;
  for (int j = 0; j < 8; j++) dst[j] = line[j];
}

}  // namespace

// The tables of one reference, hashed once and shared by every context and replica of the index: the reference shares one HashBlock_Database
// between all AlignerWorkers of a run through per-thread views (HashBlock_Database.java:129-133, Mapper.java:1026-1040, Api.java:78).
struct HostShare {
  HostIndex host;
  std::mutex mu;                     // growth of the host tables (Readable_HashBlock_Database.getContainingMap, :108-113), save
  std::atomic<int> hashedLength{0};  // copy of host.maxHashedLength readable without mu
};

// The same tables in one GPU's HBM: one per (index, device), shared by every context of the index on that GPU.
struct DeviceTables {
  std::shared_ptr<HostShare> hs;
  int device = 0;
  std::shared_mutex rw;      // align / probe calls of any number of contexts hold it shared while their kernels read the tables; (re)upload holds it exclusive
  std::mutex allocMu;        // contexts of one GPU size and allocate their scratch one after the other (they all look at the same free memory)
  std::atomic<int> uploadedLength{-1};   // host.maxHashedLength the device tables hold (written under hs->mu + rw, read without them by ensureTablesFor's first test)
  std::atomic<int> contexts{0};  // handles that share these tables (contexts of this GPU): a context sizes its launches for its share of the wave slots
  DevBuf<int64_t> dContigStart, dSeqCumStart, dDupKeyStart;
  DevBuf<int32_t> dContigLen, dDupKeys;
  DevBuf<uint8_t> dRefCodes;
  DevBuf<Table> dTables;
  DevBuf<uint32_t> dBucketOff, dPositions32;
  DevBuf<uint64_t> dPositions64;
  DevBuf<int32_t> dBaLogStep;
  DevBuf<uint32_t> dLines32;  // bucket lines (IndexView::lines32 / lines64), built on the device from the CSR tables by upload()
  DevBuf<uint64_t> dLines64;
  bool posIs64 = false;
  IndexView view;
  int numCUs = 0;
  // The one staging stream of this GPU (xm_batch_stage): made by the first batch staged, shared by every context - a batch's copy is a few per cent of its
  // alignment, so the contexts' copies can queue behind each other - and kept until the tables go, whichever context made it.  The tables keep no other
  // stream: the runtime spreads a process's live streams over a few hardware queues, and launches of streams that share one run one after the other.
  std::mutex copyMu;         // creation of copyStream, and one batch's copies at a time on it
  hipStream_t copyStream = nullptr;
  // queue(stream) under the lock: the copies of one batch, queued together (the caller has allocated; nothing here waits for the device)
  template <class Queue>
  void onStagingStream(Queue&& queue) {
    std::lock_guard<std::mutex> lock(copyMu);
    if (!copyStream) HIP_CHECK(hipStreamCreateWithFlags(&copyStream, hipStreamNonBlocking));
    queue(copyStream);
  }

  // Host tables -> HBM (caller holds hs->mu and rw exclusively).  With `peer` (a replica on another GPU): the tables are copied from the peer's HBM
  // instead (hipMemcpyPeer: over xGMI), not sent over PCIe a second time.
  void upload(const DeviceTables* peer = nullptr) {
    const HostIndex& host = hs->host;
    HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    numCUs = prop.multiProcessorCount;
    auto up = [&](auto& buf, const auto& vec, const auto& peerBuf) {
      buf.ensure(vec.size());
      if (vec.empty()) return;
      if (peer) HIP_CHECK(hipMemcpyPeer(buf.p, device, peerBuf.p, peer->device, vec.size() * sizeof(vec[0])));
      else HIP_CHECK(hipMemcpy(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice));
    };
    const DeviceTables& src = peer ? *peer : *this;
    up(dContigStart, host.contigStart, src.dContigStart); up(dContigLen, host.contigLen, src.dContigLen); up(dSeqCumStart, host.seqCumStart, src.dSeqCumStart);
    up(dRefCodes, host.refCodes, src.dRefCodes); up(dTables, host.tables, src.dTables); up(dBucketOff, host.bucketOff, src.dBucketOff);
    up(dDupKeyStart, host.dupKeyStart, src.dDupKeyStart); up(dDupKeys, host.dupKeys, src.dDupKeys);
    // (XM_FORCE_POS64=1: test hook, the 64-bit position arrays of references beyond 2^32 encoded positions on a small reference)
    posIs64 = peer ? peer->posIs64 : (host.seqCumStart.back() > 0xFFFFFFFFll || envInt("XM_FORCE_POS64", 0) != 0);
    if (posIs64) {
      up(dPositions64, host.positions, src.dPositions64);
    } else if (peer) {
      dPositions32.ensure(host.positions.size());
      if (!host.positions.empty()) HIP_CHECK(hipMemcpyPeer(dPositions32.p, device, peer->dPositions32.p, peer->device, host.positions.size() * sizeof(uint32_t)));
    } else {
      std::vector<uint32_t> p32(host.positions.size());
      for (size_t i = 0; i < p32.size(); i++) p32[i] = (uint32_t)host.positions[i];
      up(dPositions32, p32, dPositions32);
    }
    // bucket lines: 32 bytes (64 with 64-bit positions) per bucket, when they fit beside the index (XM_INDEX_LINES=0: CSR probes only)
    view.lines32 = nullptr; view.lines64 = nullptr;
    dLines32.release(); dLines64.release();
    if (envInt("XM_INDEX_LINES", 1) != 0 && !host.bucketOff.empty()) {
      const size_t words = host.bucketOff.size() * 8;
      size_t freeB = 0, totalB = 0;
      const size_t need = words * (posIs64 ? 8 : 4);
      if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && need < freeB / 2) {
        if (posIs64) dLines64.ensure(words); else dLines32.ensure(words);
        // a stream for the life of this upload (a blocking one: its kernels run behind the copies above, which went through the null stream)
        struct UploadStream {
          hipStream_t s = nullptr;
          ~UploadStream() { if (s) (void)hipStreamDestroy(s); }
        } us;
        HIP_CHECK(hipStreamCreate(&us.s));
        hipStream_t stream = us.s;
        for (const Table& t : host.tables) {
          if (t.capacity < 1) continue;
          const unsigned grid = (unsigned)(((long long)t.capacity + 255) / 256);
          if (posIs64) hipLaunchKernelGGL((xm_lines_kernel<uint64_t, uint64_t>), dim3(grid), dim3(256), 0, stream, t, (const uint32_t*)dBucketOff.p, (const uint64_t*)dPositions64.p, dLines64.p);
          else hipLaunchKernelGGL((xm_lines_kernel<uint32_t, uint32_t>), dim3(grid), dim3(256), 0, stream, t, (const uint32_t*)dBucketOff.p, (const uint32_t*)dPositions32.p, dLines32.p);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
        view.lines32 = dLines32.p; view.lines64 = dLines64.p;
      }
    }
    fillHostFields(view, host, posIs64);
    view.contigStart = dContigStart.p; view.contigLen = dContigLen.p; view.seqCumStart = dSeqCumStart.p; view.refCodes = dRefCodes.p;
    view.tables = dTables.p; view.bucketOff = dBucketOff.p; view.positions32 = dPositions32.p; view.positions64 = dPositions64.p;
    view.dupKeyStart = dDupKeyStart.p; view.dupKeys = dDupKeys.p;
    view.conf = nullptr; view.confMask = 0; view.confMiss = nullptr;  // (per call: alignResidentLocked)
    {
      int32_t steps[24];
      blockAlignerLogSteps(steps, 24);
      dBaLogStep.ensure(24);
      HIP_CHECK(hipMemcpy(dBaLogStep.p, steps, sizeof(steps), hipMemcpyHostToDevice));
      view.baLogStep = dBaLogStep.p;
    }
    uploadedLength = host.maxHashedLength;
    hs->hashedLength.store(host.maxHashedLength);
  }
  ~DeviceTables() {
    (void)hipSetDevice(device);
    if (copyStream) (void)hipStreamDestroy(copyStream);
  }
};

// One batch of queries in HBM: what the kernels read through BatchView, and what the host knows about it.
struct DeviceBatch {
  DevBuf<int32_t> mateCount, mateLength;
  DevBuf<int64_t> mateOffset;
  DevBuf<uint8_t> codes;
  DevBuf<double> expected, deviation;
  DevBuf<char> names;         // the mates' names as xm_batch_stage_fastq built them (xmio_batch's layout: nameOff has 2 * nq + 1 entries), for xm_sam_format_last;
  DevBuf<int64_t> nameOff;    // they belong to the batch, so that they swap with it in xm_batch_commit while the next block is staged
  bool hasNames = false;      // false: a batch copied in from arrays, which have no names
  DevBuf<char> quals;         // the mates' quality strings the same way (xm_fastq_text.keep_qualities), for xm_unaligned_format_last: staging block k + 1 must not
  DevBuf<int64_t> qualOff;    // overwrite them while batch k is resident, so they change hands in xm_batch_commit as the names do; hasQual[2 * nq]: the mate
  DevBuf<uint8_t> hasQual;    // came as FASTQ (written by every parse, with or without kept qualities)
  bool hasQuals = false;      // true: quals, qualOff and hasQual hold this batch's qualities
  int64_t codesLength = 0, namesLength = 0, qualsLength = 0;  // the bytes of codes, names and quals that are this batch's (a batch staged from text)
  int64_t nq = -1;            // -1: no batch
  int maxLen = 0;             // longest mate
  bool anyPaired = false;
  double h2dMs = 0;
  std::vector<int32_t> lens;  // distinct total query lengths, ascending (the confidence table is seeded for them)
  // host -> HBM, timed between the two events (the caller has validated b); a copy that throws leaves "no batch".  withStream(queue) calls queue(stream) with the
  // stream the copies go to - the context's own, or the GPU's staging stream under its lock (DeviceTables::onStagingStream).  The buffers are allocated before
  // that (a buffer that grows frees the old one, which waits for the device), and the wait is for this batch's last copy, not for the stream.
  template <class WithStream>
  void copyIn(const xm_query_batch* b, hipEvent_t e0, hipEvent_t e1, WithStream&& withStream) {
    const int64_t n = b->num_queries;
    nq = -1;
    h2dMs = 0;
    hasNames = false;
    hasQuals = false;
    if (n > 0) {
      mateCount.ensure((size_t)n); mateOffset.ensure((size_t)n * 2); mateLength.ensure((size_t)n * 2);
      codes.ensure((size_t)b->codes_length); expected.ensure((size_t)n); deviation.ensure((size_t)n);
      withStream([&](hipStream_t s) {
        HIP_CHECK(hipEventRecord(e0, s));
        HIP_CHECK(hipMemcpyAsync(mateCount.p, b->mate_count, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(mateOffset.p, b->mate_offset, sizeof(int64_t) * (size_t)n * 2, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(mateLength.p, b->mate_length, sizeof(int32_t) * (size_t)n * 2, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(codes.p, b->codes, (size_t)b->codes_length, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(expected.p, b->expected_inner, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(deviation.p, b->deviation, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipEventRecord(e1, s));
      });
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      h2dMs = ms;
    }
    nq = n;
  }
  BatchView view() const { return BatchView{nq, mateCount.p, mateOffset.p, mateLength.p, codes.p, expected.p, deviation.p}; }
};

// What xm_batch_stage_fastq works with besides the staged batch (xm_fastq.h; xm_capi_fastq.h): the text of a block in HBM, the line ends and the fields of its
// records, the scans' block sums (the names and the qualities are the batch's: DeviceBatch).  Empty until the first such call of the context.
struct FastqStage {
  DevBuf<char> dText[2];
  DevBuf<int32_t> dLineEnd[2], dTileCount[2];
  DevBuf<FastqMate> dMates;
  DevBuf<long long> dBlockSums;
  DevBuf<FastqCtl> dCtl;
  DevBuf<FastqMate> dRecs;        // the split form (split_past_size > 0): the fields of every record, its section count, its first query, the scan's block sums
  DevBuf<int32_t> dRecCount;
  DevBuf<int64_t> dRecFirst;
  DevBuf<long long> dRecBlockSums;
  DevBuf<int32_t> dLineStart[2], dLineBases[2], dBaseBefore[2], dRecLine[2];  // FASTA text (xm_batch_stage_fasta; xm_fasta.h): the per-line arrays of each text, its records' header lines,
  DevBuf<uint8_t> dLineHeader[2];                                             // the line scans' block sums
  DevBuf<long long> dLineBlockSums[2];
  // on the GPU's staging stream: text up | stages 1-3 | (host sizes the arrays) | stage 4 | arrays down; the split form also [6] behind stage 2b and [7] in front of 2c (the host sizes the slots between them)
  StageEvents<8> ev;
};

// What xm_sam_format_last works with (xm_sam.h; xm_capi_sam.h): the contig names, uploaded once per context; names the host handed in for a call; bytes and
// records per query, the scan's block sums and the offsets; the control words; the text, which only grows; the call's events on the context's stream.
struct SamStage {
  int32_t numContigs = -1;     // -1: xm_sam_set_contigs has not been called
  DevBuf<char> dContigNames, dNames, dText;
  DevBuf<int64_t> dContigOff, dNameOff;
  DevBuf<long long> dBytes, dRecords, dBlockSums, dOffset;
  DevBuf<unsigned long long> dCtl;
  StageEvents<6> ev;  // names up | measure and offsets | (host sizes the text) | write | text down
};

// What xm_summary_last works with (xm_summary.h; xm_capi_summary.h): alignments and the unaligned flag per query, the scan's block sums and both offset arrays;
// the control word and the three counters; the penalties and the list of unaligned queries, which only grow; the call's events on the context's stream.
struct SummaryStage {
  DevBuf<int32_t> dAlignments, dUnalignedFlag;
  DevBuf<long long> dBlockSums;
  DevBuf<int64_t> dOff, dUoff, dUnaligned;
  DevBuf<unsigned long long> dCtl;
  DevBuf<double> dPenalties;
  StageEvents<5> ev;  // measure and offsets | (host sizes the arrays) | gather | arrays down
};

// What xm_unaligned_format_last works with (xm_unaligned.h; xm_capi_unaligned.h): the record bytes and the unaligned flag per query, the scan's block sums and
// both offset arrays; the control words; the list of unaligned queries and the text, which only grow; the call's events on the context's stream.  Nothing is
// allocated before the first call.
struct UnalignedStage {
  DevBuf<int32_t> dBytes, dFlag;
  DevBuf<long long> dBlockSums;
  DevBuf<int64_t> dOff, dUoff, dList;
  DevBuf<unsigned long long> dCtl;
  DevBuf<char> dText;
  StageEvents<5> ev;  // measure and offsets | (host sizes the list and the text) | compact and write | text down
};

// What xm_refs_count_last works with (xm_refs.h; xm_capi_refs.h): the table of the sets' fingerprints (keys, the lowest query and the count per slot); per query
// its slot, whether it is its slot's representative, and what it leaves to the host (a flag and its sequence alignments); the scan's block sums and the three
// offset arrays; the control words; the records and the left-over contigs with their starts, which only
// grow; the call's events on the context's stream.  Nothing is allocated before the first call.
struct RefsStage {
  DevBuf<unsigned long long> dKeys, dReps, dCounts, dCtl;
  DevBuf<int32_t> dSlotOf, dIsRep, dLeftLen, dLeftFlag, dLeft;
  DevBuf<long long> dBlockSums;
  DevBuf<int64_t> dOff, dLoff, dLqoff, dLeftStart;
  DevBuf<RefsRecord> dRecords;
  StageEvents<5> ev;  // claim, verify and offsets | (host sizes the arrays) | gather | arrays down
};

// What the lane-per-read passes of a call work with besides the batch and the result stage: the work lists the lanes file unfinished reads into and the
// counts of those lists (PassLists, PassCtl: xm_kernel_common.h), the device counters, and the scratch - the lanes' arenas behind the pool of saved
// regions (HandOver), a wave's search nodes, the pool of search buffers (SearchPool).  Kept across calls; which list a pass reads is xm_pass_plan.h's.
struct PassBuffers {
  DevBuf<int64_t> dListHeavy, dListHeavyLate, dListScale[2], dListOut[2], dListConf[2];
  DevBuf<PassCtl> dCtl;
  DevBuf<DevCounters> dCounters;
  DevBuf<uint8_t> dArenas;      // [region pool | lane arenas] (LaunchPlan)
  DevBuf<int32_t> dRegionOf;
  DevBuf<PNode> dWaveNodes;     // per wave: node payloads of its LDS-mode search
  DevBuf<uint8_t> dSearchPool;  // one buffer per wave for the arrays of HBM-mode searches (SearchPool, xm_extend.h)
  DevBuf<LaunchConst> dLaunchConst;  // what every lane of a launch reads and none keeps (xm_defs.h); the context's own: contexts of one index run with different parameters

  // The block of the next launch, written on s behind whatever launch of this context read the last one.  The view changes between the passes of a call (a
  // confidence rerun: the table grew and moved), the parameters from call to call.  (params: as the lanes use them, StartingInsertionStartFree 0.)
  const LaunchConst* launchConst(const IndexView& view, const Params& params, hipStream_t s) {
    dLaunchConst.ensure(1);
    const LaunchConst lc = launchConstOf(view, params);
    HIP_CHECK(hipMemcpyAsync(dLaunchConst.p, &lc, sizeof(lc), hipMemcpyHostToDevice, s));
    return dLaunchConst.p;
  }

  // sized for a call of nq queries; counters and counts cleared, no query in error
  void prepare(int64_t nq, hipStream_t s) {
    dListConf[0].ensure((size_t)nq); dListConf[1].ensure((size_t)nq);
    dCounters.ensure(1); dCtl.ensure(1);
    dListHeavy.ensure((size_t)nq); dListHeavyLate.ensure((size_t)nq);
    HIP_CHECK(hipMemsetAsync(dCounters.p, 0, sizeof(DevCounters), s));
    PassCtl ctl0;
    memset(&ctl0, 0, sizeof(ctl0));
    ctl0.errQuery = ~0ull;
    HIP_CHECK(hipMemcpyAsync(dCtl.p, &ctl0, sizeof(ctl0), hipMemcpyHostToDevice, s));
  }
  void forgetRegions(int64_t nq, hipStream_t s) {  // (calls with the hand-over: no read has a saved region)
    dRegionOf.ensure((size_t)nq);
    HIP_CHECK(hipMemsetAsync(dRegionOf.p, 0xFF, sizeof(int32_t) * (size_t)nq, s));
  }
  // the lists a pass in state st files into: the lanes file the reads they could not finish into the work lists of the passes to come as they publish them
  // (no kernel behind the pass)
  PassLists lists(const PassState& st, int64_t nq, int heavyHint) {
    dListScale[st.ts].ensure((size_t)nq); dListOut[st.to].ensure((size_t)nq);
    return PassLists{dListHeavy.p, dListHeavyLate.p, dListScale[st.ts].p, dListOut[st.to].p, dListConf[st.tc].p, heavyHint, st.ts, st.to, st.tc, dCtl.p};
  }
  // light pass -> gapped pass hand-over (HandOver, SavedRead): the reads the light pass stops in front of the gapped chain keep their seeding
  // state in HBM and the gapped pass continues from it
  HandOver handOver(const BatchPolicy& pol, const PassState& st, const LaunchPlan& pl, unsigned long long* regionCursor) const {
    return HandOver{st.hoMode, pol.seedScale, dArenas.p, (unsigned long long)pol.regionBytes, pl.nRegions, dRegionOf.p, regionCursor};
  }
  SearchPool searchPool(const PassState& st, const LaunchPlan& pl) {
    SearchPool pool{nullptr, 0, 0, 0};
    if (pl.poolBuffers > 0) {
      pool.bufBytes = searchPoolBytes(makeCaps(st.scale));
      pool.n = (int32_t)pl.poolBuffers;
      dSearchPool.ensure((size_t)pool.n * pool.bufBytes);
      pool.base = dSearchPool.p;
    }
    return pool;
  }
  // The list nextPass chose for the next launch (np.kind is not Done; ctl: the counts the last launch left).  The count of the half that launch files into
  // is cleared on s; the gapped pass gets the late list appended to the heavy one, and both their counts cleared (a gapped pass never adds to these lists).
  const int64_t* take(const NextPass& np, const PassCtl& ctl, hipStream_t s) {
    unsigned long long* count = nullptr;
    const int64_t* list = nullptr;
    switch (np.kind) {
      case PassKind::Done: break;
      case PassKind::OutRerun: list = dListOut[np.list].p; count = &dCtl.p->nOut[np.clear]; break;
      case PassKind::ConfRerun: list = dListConf[np.list].p; count = &dCtl.p->nConf[np.clear]; break;
      case PassKind::ScaleRerun: list = dListScale[np.list].p; count = &dCtl.p->nScale[np.clear]; break;
      case PassKind::Gapped:
        if (ctl.nHeavyLate > 0) HIP_CHECK(hipMemcpyAsync(dListHeavy.p + ctl.nHeavy, dListHeavyLate.p, sizeof(int64_t) * (size_t)ctl.nHeavyLate, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemsetAsync(&dCtl.p->nHeavy, 0, 2 * sizeof(unsigned long long), s));  // nHeavy, nHeavyLate
        return dListHeavy.p;
    }
    if (count) HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
    return list;
  }
};

// The confidence table of a context (IndexView::conf): the host's table (xm_conf_table.h), its copy in HBM, the list the kernels leave the keys in that
// the table did not hold.
struct DeviceConfTable {
  ConfTable host;
  static constexpr size_t kMissCap = 1 << 16;
  DevBuf<ConfEntry> dConf;
  DevBuf<uint8_t> dConfMiss;   // ConfMiss: header and kMissCap keys

  // the copy in HBM brought up to the host's
  void upload(hipStream_t s) {
    if (!host.dirty()) return;
    HIP_CHECK(hipStreamSynchronize(s));   // (no kernel of this context reads the old copy any more)
    dConf.ensure(host.size());
    HIP_CHECK(hipMemcpy(dConf.p, host.data(), host.size() * sizeof(ConfEntry), hipMemcpyHostToDevice));
    host.markUploaded();
  }
  // the table of one align call (ConfTable::prepare) in HBM, and an empty miss list (its header is written once: absorbMisses leaves it empty)
  void prepare(const Params& params, const std::vector<int32_t>& lens, double granularity, int64_t totalSize, long long seedBudget, hipStream_t s) {
    host.prepare(params, lens, granularity, totalSize, seedBudget);
    upload(s);
    if (dConfMiss.p) return;
    dConfMiss.ensure(sizeof(ConfMiss) + kMissCap * sizeof(ConfMissKey));
    ConfMiss hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.cap = kMissCap;
    HIP_CHECK(hipMemcpyAsync(dConfMiss.p, &hdr, offsetof(ConfMiss, keys), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  // after a pass with XM_ST_NEED_CONF reads: the keys they left in the miss list, evaluated and added
  void absorbMisses(hipStream_t s) {
    ConfMiss hdr;
    HIP_CHECK(hipMemcpyAsync(&hdr, dConfMiss.p, offsetof(ConfMiss, keys), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t n = (size_t)std::min<unsigned long long>(hdr.n, hdr.cap);
    std::vector<ConfMissKey> keys(n);
    if (n) HIP_CHECK(hipMemcpy(keys.data(), dConfMiss.p + offsetof(ConfMiss, keys), n * sizeof(ConfMissKey), hipMemcpyDeviceToHost));
    const unsigned long long zero = 0;
    HIP_CHECK(hipMemcpy(dConfMiss.p, &zero, sizeof(zero), hipMemcpyHostToDevice));
    for (const ConfMissKey& k : keys) { double pen; memcpy(&pen, &k.penaltyBits, 8); host.insert(pen, k.queryLength); }
    upload(s);
  }
  // the three fields of a call's IndexView (again after absorbMisses: the table may have grown and moved)
  void fillView(IndexView& v) const { v.conf = dConf.p; v.confMask = host.mask(); v.confMiss = (ConfMiss*)dConfMiss.p; }
};

// what only the wave-per-read passes use (runWaveForm)
struct WaveFormBuffers {
  DevBuf<int64_t> dListWaveHeavy, dListWaveNext, dListWaveSearch[2], dListFallback;
  DevBuf<uint8_t> dWaveMemo;
  DevBuf<int32_t> dWaveSlotOf;
  DevBuf<WaveCtl> dWaveCtl;
  DevBuf<uint8_t> dWaveArenas;
  DevBuf<PNode> dWaveNodes2;
};
// collapsing of identical queries (xm_collapse.h; allocated only when it is on): fingerprint table, query -> representative, the representatives, block counts
struct CollapseBuffers {
  DevBuf<unsigned long long> dCollapseKeys, dCollapseReps, dCollapseTotal;
  DevBuf<int64_t> dRepOf, dRepList;
  DevBuf<long long> dCollapseBlocks;
};
// the run-wide memory of aligned queries (xm_memory_new: one per GPU, shared by the contexts attached to it; xm_context_set_memo: a private one of one
// generation; xm_memo.h, xm_memo_plan.h).  What a stored result depends on
// besides the query: the index - a memory belongs to the tables of one index on one GPU; the parameters - `filledUnder`, memoMustEmpty; and NOT the hashed length: a read only probes the
// tables of gapmer lengths up to its own length, those tables never change once they are hashed (growth adds tables of greater lengths), and a read that
// needs a table that is not there fails its call (XM_ST_NEED_GROW; ensureTablesFor makes that unreachable through the batch entries) instead of aligning
// differently.  So the memory survives xm_index_ensure_length and growth by another context.  A call that throws never reaches the insert.
//
// THE ONE CONCURRENCY RULE: launches of different contexts never touch a memory at the same time.  A call holds `mu` twice: (a) from before its lookup until
// replay and promotion have completed on its stream (the sizing of the result arenas between lookup and replay is inside), and (b) from before the measure
// kernel until the insert (and a turn's clears) have completed on its stream.  Between (a) and (b), while the passes run, `mu` is free: the contexts of a
// GPU keep overlapping their passes.  A call carries nothing across that gap but fp[] and its own results: another context may have inserted the same key
// meanwhile (the claim drops it), turned the generations, or emptied the memory for other parameters.  Lock order: the context's mu, then the memory's.
struct Memory {
  std::mutex mu;
  int device = 0;
  std::weak_ptr<DeviceTables> dt;   // the tables its records were aligned against (only their contexts attach)
  std::weak_ptr<HostShare> hs;
  bool isPrivate = false;           // xm_context_set_memo's: one context, one generation
  MemoPlan plan{0, 0, 0};           // of one generation
  MemoGenerations gens;             // the host's copy of dState after the last launch that changed it, which generation is young, turns, promotions
  int fingerprintBits = 64;
  DevBuf<unsigned long long> dKeys, dOffs, dState;  // [generations * slots], [generations * slots], [generations * 4]
  DevBuf<uint8_t> dArena;                           // [generations * arenaBytes]
  int64_t timesEmptied = 0;
  bool filled = false;              // something was inserted under `filledUnder`
  xm_params filledUnder;
  std::atomic<int> attached{0};     // contexts that look their queries up here
  MemoView view() const {
    return MemoView{dKeys.p, dOffs.p, (unsigned long long)plan.slots - 1, dArena.p, (unsigned long long)plan.arenaBytes, dState.p, fingerprintBits, gens.generations, gens.young};
  }
  void allocate(const MemoPlan& p, int generations) {
    const size_t g = (size_t)generations;
    dKeys.ensure(g * (size_t)p.slots); dOffs.ensure(g * (size_t)p.slots); dState.ensure(g * 4); dArena.ensure(g * (size_t)p.arenaBytes);
    plan = p;
    gens = MemoGenerations();
    gens.generations = generations;
  }
  void clearGeneration(int g, hipStream_t s) {  // every slot empty, nothing in the arena (enqueued on s: the caller waits for s before it lets go of mu)
    HIP_CHECK(hipMemsetAsync(dKeys.p + (size_t)g * (size_t)plan.slots, 0, sizeof(unsigned long long) * (size_t)plan.slots, s));
    HIP_CHECK(hipMemsetAsync(dOffs.p + (size_t)g * (size_t)plan.slots, 0xFF, sizeof(unsigned long long) * (size_t)plan.slots, s));
    HIP_CHECK(hipMemsetAsync(dState.p + (size_t)g * 4, 0, sizeof(unsigned long long) * 4, s));
    memoEmptyGeneration(gens, g);
  }
  void clear(hipStream_t s) {
    for (int g = 0; g < gens.generations; g++) clearGeneration(g, s);
    filled = false;
  }
  ~Memory() {
    (void)hipSetDevice(device);
    dKeys.release(); dOffs.release(); dState.release(); dArena.release();
  }
};
// what belongs to a call stays with the context: where each representative's record is, its fingerprint, the ones that missed, the control words
struct MemoCallBuffers {
  DevBuf<unsigned long long> dTotals, dFp;  // dTotals: [0..2] hits, their ints, their doubles, [3] replays without room, [4..5] old-generation hits and their bytes (then: what the insert measures), [6] promoted
  DevBuf<int64_t> dHit, dMissList;
};

// An xm_index handle is a CONTEXT of an index: what one host thread needs to align batches on one GPU - a stream, batch buffers, scratch and a
// result pool of its own - over tables it shares with every other context of the same index (HostShare: all of them; DeviceTables: those on
// its GPU).  xm_index_build / xm_index_load make the first context; xm_context_new and xm_index_replicate add contexts.
struct xm_index {
  std::shared_ptr<HostShare> hs;
  std::shared_ptr<DeviceTables> dt;  // null with host_only
  bool hostOnly = false;
  int device = 0;
  long long scratchBytes = 0;        // xm_context_set_scratch: upper limit of this context's scratch (0: XM_SCRATCH_GIB / the default)
  bool collapse = false;             // xm_context_set_collapse: identical queries of a batch are aligned once (xm_collapse.h)
  std::mutex mu;                     // calls on one context serialise; contexts run side by side
  HostIndex& host() { return hs->host; }
  const HostIndex& host() const { return hs->host; }
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // what a call works with, kept across calls: every device buffer of a context belongs to one of these, to memoCall or to a batch below
  ResultStage results;
  PassBuffers passes;
  DeviceConfTable conf;
  WaveFormBuffers wave;
  CollapseBuffers collapseBufs;
  std::shared_ptr<Memory> memo;      // xm_context_attach_memory / xm_context_set_memo: where this context looks its queries up and remembers what it aligns (null: nowhere)
  MemoCallBuffers memoCall;
  int64_t memoEmptiedBefore = 0;     // xm_context_memo_info's out[3] over the private memories this context has had
  bool memoOn() const { return (bool)memo; }
  void dropMemo() {                  // (caller holds mu; the stream is idle)
    if (memo) { if (memo->isPrivate) memoEmptiedBefore = memo->timesEmptied; memo->attached.fetch_sub(1); }
    memo.reset();
    memoCall = MemoCallBuffers();
  }
  // the batch the align calls work on (xm_batch_upload, xm_batch_commit), and the one xm_batch_stage copies in on its own stream meanwhile
  DeviceBatch resident, staged;
  int64_t residentGen = 0;     // which resident batch: a call's streams belong to one (ResultStage::lastStreams)
  std::mutex stageMu;
  hipEvent_t cev0 = nullptr, cev1 = nullptr;  // this context's events on the GPU's staging stream (DeviceTables::copyStream)
  FastqStage fastq;            // xm_batch_stage_fastq's buffers (under stageMu)
  SamStage sam;                // xm_sam_format_last's buffers (under mu)
  SummaryStage summary;        // xm_summary_last's buffers (under mu)
  RefsStage refs;              // xm_refs_count_last's buffers (under mu)
  bool resultCopy = true;      // xm_context_set_result_copy: an align call copies its four streams to the host (false: they stay in HBM, and the result has none)
  UnalignedStage unaligned;    // xm_unaligned_format_last's buffers (under mu)
  bool batchCopy = true;       // xm_context_set_batch_copy: a batch staged from text is copied to the host whole (false: only the mate counts, offsets and lengths; under stageMu)

  void initContext() {  // stream and events of this context (the device tables exist)
    dt->contexts.fetch_add(1);
    HIP_CHECK(hipSetDevice(device));
    if (!stream) { HIP_CHECK(hipStreamCreate(&stream)); HIP_CHECK(hipEventCreate(&ev0)); HIP_CHECK(hipEventCreate(&ev1)); }
  }
  // Readable_HashBlock_Database.getContainingMap's growth (:108-113) for a batch whose longest mate is maxLen, then the device tables brought up to
  // the host's: any context may grow the shared tables; every GPU's copy follows before its next launch.  Called without rw held.
  void ensureTablesFor(int maxLen) {
    if (maxLen > hs->hashedLength.load()) {
      std::lock_guard<std::mutex> lock(hs->mu);
      if (maxLen > hs->host.maxHashedLength) { hs->host.ensureLength(maxLen); hs->hashedLength.store(hs->host.maxHashedLength); }
    }
    if (dt && dt->uploadedLength < hs->hashedLength.load()) {
      std::lock_guard<std::mutex> lock(hs->mu);
      std::unique_lock<std::shared_mutex> wr(dt->rw);  // (waits for the launches of every context of this GPU)
      if (dt->uploadedLength < hs->host.maxHashedLength) dt->upload();
    }
  }
  ~xm_index() {
    if (dt) dt->contexts.fetch_sub(1);
    if (hostOnly) return;
    (void)hipSetDevice(device);
    if (memo) memo->attached.fetch_sub(1);  // (the memory itself goes with its last holder: the handle or a context)
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (cev0) (void)hipEventDestroy(cev0);
    if (cev1) (void)hipEventDestroy(cev1);
    if (stream) (void)hipStreamDestroy(stream);
  }  // (every DevBuf member releases its memory itself; the shared tables go with their last context)
};

// What every C entry that reads the last align call's result streams where they lie in HBM begins with (caller holds idx->mu): the streams, or the error of a
// context whose resident batch is no longer the one they belong to; behind it the context's device is current.
static ResultStage::LastStreams lastCall(xm_index* idx, const char* entry) {
  const ResultStage::LastStreams last = idx->results.lastStreams(idx->residentGen, idx->resident.nq);
  if (last.nq < 0)
    throw std::runtime_error(std::string("the batch of the last align call is no longer resident (call ") + entry +
                             " after xm_align_batch / xm_align_resident, before the next batch is uploaded or committed)");
  HIP_CHECK(hipSetDevice(idx->device));
  return last;
}
// ... and the frame around it for the entries that hand back one object: *out = body(), run under the context's mutex; what body throws is the entry's error.
template <class Out, class Body>
static int lastCallEntry(xm_index* idx, Out** out, const char* entry, Body&& body) {
  if (!idx || !out) return fail(std::string(entry) + ": null argument");
  *out = nullptr;
  if (idx->hostOnly) return fail(std::string(entry) + ": index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    *out = body();
    return 0;
  } catch (std::exception& e) { return fail(std::string(entry) + ": " + e.what()); }
}

// ---------------------------------------------------------------- the align call: its state and its steps, in the order alignResidentLocked runs them
// (what the passes are sized by and how they follow each other is xm_pass_plan.h; here are the buffers, the launches and the copies)
struct AlignCall {
  xm_index* idx;
  ResultBox* box;
  xm_result* res;
  int64_t nq;
  hipStream_t s;
  int numCUs;
  IndexView view;
  Params params;
  xm_params cParams;                 // the caller's, bit for bit (what the run-wide memory is filled under)
  BatchView bv;
  const int64_t* todo = nullptr;  // device list of the current pass; null on the first pass = all reads
  long long nTodo = 0;
  double kernelMs = 0;
  int launches = 0;
  int64_t copies = 0, rerun = 0;
  int64_t remembered = 0;            // representatives served from the run-wide memory (Memory)
  unsigned long long hitInts = 0, hitDbls = 0;  // what their slices need in the result arenas
  unsigned long long oldHits = 0, oldHitBytes = 0;  // the ones served from the old generation only, the bytes of their records (memoPromotes)
  long long nMisses = 0;             // idx->memoCall.dMissList: the representatives this call aligns
  double memoWaitUs = 0;             // host time this call waited for the memory's mutex (both critical sections)
  bool boundFilterUsed = false;
#ifdef XM_READ_TIMES
  DevBuf<unsigned long long> dReadTimes;
  const char* readTimesFile = nullptr;
#endif
};

// One timed step on the call's stream: record, launch(es), hipGetLastError, record, `after` (enqueues the copies of the control words the host reads
// next), synchronise.  The milliseconds between the events go to kernel_ms and, with a slot, to counters[slot] as microseconds.
template <class Launch, class After>
static float timedLaunch(AlignCall& c, int nKernels, int slot, Launch&& launch, After&& after) {
  float ms = 0;
  HIP_CHECK(hipEventRecord(c.idx->ev0, c.s));
  launch();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(c.idx->ev1, c.s));
  after();
  HIP_CHECK(hipStreamSynchronize(c.s));
  HIP_CHECK(hipEventElapsedTime(&ms, c.idx->ev0, c.idx->ev1));
  c.kernelMs += ms;
  if (slot >= 0) c.res->counters[slot] += (int64_t)(ms * 1000.0);
  c.launches += nKernels;
  return ms;
}

// buffers that follow the batch's size, the confidence table of these parameters, cleared counters and control words
static void prepareCall(AlignCall& c) {
  xm_index* idx = c.idx;
  const int64_t nq = c.nq;
  hipStream_t s = c.s;
  // (XM_CONF_SEED = 0: nothing seeded, every key through the miss path - the tests run that)
  idx->conf.prepare(c.params, idx->resident.lens, idx->host().dupGranularity(), idx->host().totalForwardSize * 2, envKnob("XM_CONF_SEED", 1 << 18, 0, 1 << 26), s);
  idx->conf.fillView(c.view);
  idx->results.prepare(nq, s);
  idx->passes.prepare(nq, s);
#ifdef XM_READ_TIMES
  c.readTimesFile = getenv("XM_READ_TIMES_FILE");
  if (c.readTimesFile && *c.readTimesFile) {
    c.dReadTimes.ensure((size_t)nq);
    HIP_CHECK(hipMemset(c.dReadTimes.p, 0, sizeof(unsigned long long) * (size_t)nq));
    HIP_CHECK((hipError_t)xmSetReadTimes(c.dReadTimes.p));
  }
#endif
  c.todo = nullptr;
  c.nTodo = nq;
}

// the queries of the batch that xmListed lists (hit: null, or the memory's look-up of the representatives) in ascending order -> list, their number ->
// dCollapseTotal; three launches enqueued on s (collapseBuildList has sized the block sums for the batch)
static void collapseList(CollapseBuffers& b, int64_t nq, const int64_t* hit, int64_t* list, hipStream_t s) {
  xmScan(CollapseListed{nq, b.dRepOf.p, hit, list, b.dCollapseTotal.p}, nq, b.dCollapseBlocks, s);
}

// identical queries (xm_context_set_collapse): the first pass gets the representatives, the lowest query index of each group of byte-identical queries,
// in ascending order (xm_collapse.h).  Every later list is built by the passes from the reads they ran: representatives only.
static void collapseBuildList(AlignCall& c) {
  xm_index* idx = c.idx;
  const int64_t nq = c.nq;
  hipStream_t s = c.s;
  size_t cap = 64;
  while (cap < (size_t)nq * 2) cap <<= 1;
  idx->collapseBufs.dCollapseKeys.ensure(cap); idx->collapseBufs.dCollapseReps.ensure(cap); idx->collapseBufs.dCollapseTotal.ensure(1);
  idx->collapseBufs.dRepOf.ensure((size_t)nq); idx->collapseBufs.dRepList.ensure((size_t)nq); idx->collapseBufs.dCollapseBlocks.ensure(xmScanSums(nq, 1));
  HIP_CHECK(hipMemsetAsync(idx->collapseBufs.dCollapseKeys.p, 0, sizeof(unsigned long long) * cap, s));
  HIP_CHECK(hipMemsetAsync(idx->collapseBufs.dCollapseReps.p, 0xFF, sizeof(unsigned long long) * cap, s));
  const unsigned waveGrid = (unsigned)((nq + 3) / 4);  // one wave per query, four per block
  unsigned long long nReps = 0;
  timedLaunch(c, 5, -1, [&] {
    hipLaunchKernelGGL(xm_collapse_fingerprint_kernel, dim3(waveGrid), dim3(256), 0, s, c.bv, idx->collapseBufs.dCollapseKeys.p, idx->collapseBufs.dCollapseReps.p, (unsigned long long)(cap - 1), idx->collapseBufs.dRepOf.p);
    hipLaunchKernelGGL(xm_collapse_verify_kernel, dim3(waveGrid), dim3(256), 0, s, c.bv, (const unsigned long long*)idx->collapseBufs.dCollapseReps.p, idx->collapseBufs.dRepOf.p);
    collapseList(idx->collapseBufs, nq, nullptr, idx->collapseBufs.dRepList.p, s);
  }, [&] { HIP_CHECK(hipMemcpyAsync(&nReps, idx->collapseBufs.dCollapseTotal.p, sizeof(nReps), hipMemcpyDeviceToHost, s)); });
  if (nReps < 1 || (long long)nReps > nq) throw std::runtime_error("internal error: collapsing found " + std::to_string(nReps) + " distinct queries in a batch of " + std::to_string(nq));
  c.copies = nq - (int64_t)nReps;
  c.todo = idx->collapseBufs.dRepList.p;
  c.nTodo = (long long)nReps;
}

// every copy's slice is its representative's: the scan and gather of finishStreams then write it in query order
static void collapseFanOut(AlignCall& c) {
  xm_index* idx = c.idx;
  timedLaunch(c, 1, -1, [&] {
    hipLaunchKernelGGL(xm_collapse_fanout_kernel, dim3((unsigned)((c.nq + 255) / 256)), dim3(256), 0, c.s, (long long)c.nq, (const int64_t*)idx->collapseBufs.dRepOf.p, idx->results.dIntOff.p, idx->results.dDblOff.p,
                       idx->results.dIntLen.p, idx->results.dDblLen.p);
  }, [] {});
}

// ---- the run-wide memory (xm_memory_new, xm_context_set_memo; Memory, xm_memo.h), in the order of a call: lookup, replay, promotion, (the passes,) measure, insert
// the memory's mutex, taken with the wait on the host's clock
static std::unique_lock<std::mutex> memoLock(AlignCall& c) {
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_lock<std::mutex> lock(c.idx->memo->mu);
  c.memoWaitUs += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  return lock;
}
// after collapseBuildList: the representatives are looked up, and the first pass's list becomes the ones the memory did not hold (caller holds the memory's mu)
static void memoLookup(AlignCall& c) {
  xm_index* idx = c.idx;
  Memory& m = *idx->memo;
  MemoCallBuffers& mc = idx->memoCall;
  const int64_t nq = c.nq;
  hipStream_t s = c.s;
  if (memoMustEmpty(m.filled, &m.filledUnder, &c.cParams, sizeof(xm_params))) { m.clear(s); m.timesEmptied++; }
  const long long nReps = c.nTodo;
  mc.dHit.ensure((size_t)nq); mc.dFp.ensure((size_t)nq); mc.dMissList.ensure((size_t)nq); mc.dTotals.ensure(8);
  HIP_CHECK(hipMemsetAsync(mc.dTotals.p, 0, sizeof(unsigned long long) * 8, s));
  unsigned long long totals[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nMisses = 0;
  timedLaunch(c, 4, -1, [&] {
    hipLaunchKernelGGL(xm_memo_lookup_kernel, dim3((unsigned)((nReps + 3) / 4)), dim3(256), 0, s, c.bv, (const int64_t*)idx->collapseBufs.dRepList.p, nReps, m.view(), mc.dHit.p, mc.dFp.p, mc.dTotals.p);
    collapseList(idx->collapseBufs, nq, mc.dHit.p, mc.dMissList.p, s);
  }, [&] {
    HIP_CHECK(hipMemcpyAsync(totals, mc.dTotals.p, sizeof(totals), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&nMisses, idx->collapseBufs.dCollapseTotal.p, sizeof(nMisses), hipMemcpyDeviceToHost, s));
  });
  if ((long long)totals[0] + (long long)nMisses != nReps)
    throw std::runtime_error("internal error: of " + std::to_string(nReps) + " distinct queries the memory held " + std::to_string(totals[0]) + " and " + std::to_string(nMisses) + " are left");
  c.remembered = (int64_t)totals[0]; c.hitInts = totals[1]; c.hitDbls = totals[2];
  c.oldHits = totals[4]; c.oldHitBytes = totals[5];
  c.nMisses = (long long)nMisses;
  c.todo = mc.dMissList.p;
  c.nTodo = c.nMisses;
}

// before the passes: the hits' slices into the result arenas, through the call's cursors (a hit is then what a read a pass finished is)
static void memoReplay(AlignCall& c) {
  xm_index* idx = c.idx;
  Memory& m = *idx->memo;
  MemoCallBuffers& mc = idx->memoCall;
  const long long nReps = c.remembered + c.nMisses;
  unsigned long long totals[4] = {0, 0, 0, 0};
  timedLaunch(c, 1, -1, [&] {
    hipLaunchKernelGGL(xm_memo_replay_kernel, dim3((unsigned)((nReps + 3) / 4)), dim3(256), 0, c.s, (const int64_t*)idx->collapseBufs.dRepList.p, nReps, m.view(), (const int64_t*)mc.dHit.p, idx->results.outView(), mc.dTotals.p);
  }, [&] {
    HIP_CHECK(hipMemcpyAsync(totals, mc.dTotals.p, sizeof(totals), hipMemcpyDeviceToHost, c.s));
    idx->results.readCursors(c.s);
  });
  if (totals[3] != 0) throw std::runtime_error("internal error: " + std::to_string(totals[3]) + " remembered results found no room in the result arenas");
}

// second chance: the records this call was served from the old generation are copied into the young one, all of them or none (memoPromotes); never a turn
static void memoPromote(AlignCall& c) {
  xm_index* idx = c.idx;
  Memory& m = *idx->memo;
  MemoCallBuffers& mc = idx->memoCall;
  if (!memoPromotes(m.plan, m.gens, c.oldHits, c.oldHitBytes)) return;
  const long long nReps = c.remembered + c.nMisses;
  const int young = m.gens.young;
  unsigned long long state[4] = {0, 0, 0, 0}, promoted = 0;
  timedLaunch(c, 1, -1, [&] {
    hipLaunchKernelGGL(xm_memo_promote_kernel, dim3((unsigned)((nReps + 3) / 4)), dim3(256), 0, c.s, (const int64_t*)idx->collapseBufs.dRepList.p, nReps, m.view(), (const int64_t*)mc.dHit.p,
                       (const unsigned long long*)mc.dFp.p, mc.dTotals.p);
  }, [&] {
    HIP_CHECK(hipMemcpyAsync(state, m.dState.p + (size_t)young * 4, sizeof(state), hipMemcpyDeviceToHost, c.s));
    HIP_CHECK(hipMemcpyAsync(&promoted, mc.dTotals.p + 6, sizeof(promoted), hipMemcpyDeviceToHost, c.s));
  });
  m.gens.claimed[young] = state[0]; m.gens.cursor[young] = state[1]; m.gens.records[young] = state[2];
  m.gens.promoted += (long long)promoted;
}

// after the last pass has succeeded: the representatives this call aligned are remembered in the young generation.  With two generations the call first
// measures what it brings (xm_memo_measure_kernel: their number and the bytes of their records) and turns the generations when the young one does not take
// all of it (memoMustTurn); with one generation nothing turns and nothing needs measuring.  Then as far as the table and the arena have room (memoInsertCount).
// Takes the memory's mu for all of it, and lets go once everything has completed on the stream.
static void memoInsert(AlignCall& c) {
  xm_index* idx = c.idx;
  Memory& m = *idx->memo;
  MemoCallBuffers& mc = idx->memoCall;
  if (c.nMisses < 1) return;
  std::unique_lock<std::mutex> lock = memoLock(c);
  bool queued = false;  // clears on the stream that no timedLaunch has waited for yet
  // (another context may have filled the memory under other parameters since this call's lookup: what this call aligned is not of them)
  if (memoMustEmpty(m.filled, &m.filledUnder, &c.cParams, sizeof(xm_params))) { m.clear(c.s); m.timesEmptied++; queued = true; }
  if (m.gens.generations > 1) {
    unsigned long long measured[2] = {0, 0};
    HIP_CHECK(hipMemsetAsync(mc.dTotals.p + 4, 0, sizeof(unsigned long long) * 2, c.s));
    timedLaunch(c, 1, -1, [&] {
      hipLaunchKernelGGL(xm_memo_measure_kernel, dim3((unsigned)((c.nMisses + 255) / 256)), dim3(256), 0, c.s, c.bv, (const int64_t*)mc.dMissList.p, c.nMisses, idx->results.outView(), mc.dTotals.p);
    }, [&] { HIP_CHECK(hipMemcpyAsync(measured, mc.dTotals.p + 4, sizeof(measured), hipMemcpyDeviceToHost, c.s)); });
    queued = false;
    if (memoMustTurn(m.plan, m.gens, measured[0], measured[1])) { m.clearGeneration(memoTurn(m.gens), c.s); queued = true; }
  }
  const long long n = memoInsertCount(m.plan, m.gens, c.nMisses);
  if (n < 1) {
    if (queued) HIP_CHECK(hipStreamSynchronize(c.s));
    return;
  }
  const int young = m.gens.young;
  unsigned long long state[4] = {0, 0, 0, 0};
  m.filledUnder = c.cParams;
  m.filled = true;
  timedLaunch(c, 1, -1, [&] {
    hipLaunchKernelGGL(xm_memo_insert_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c.s, c.bv, (const int64_t*)mc.dMissList.p, n, m.view().generation(young), (const unsigned long long*)mc.dFp.p, idx->results.outView());
  }, [&] { HIP_CHECK(hipMemcpyAsync(state, m.dState.p + (size_t)young * 4, sizeof(state), hipMemcpyDeviceToHost, c.s)); });
  m.gens.claimed[young] = state[0]; m.gens.cursor[young] = state[1]; m.gens.records[young] = state[2];
}

// ---- passes 0 (XM_WAVE=1; off by default: measured slower than the lane-per-read passes on MI355X this round, profiles/r02/NOTES.md):
// the wave-per-read form (xm_wave_kernel.hip).  Light tier over every read (seed, vote, ungapped alignment, accept); chain
// tier over the reads that need the gapped chain (or more LDS): a read that meets a PathAligner search leaves the request in its memo, the
// search kernel runs all waiting searches (one wavefront each), and those reads run again with the results, until none waits; then the
// same with the largest capacities for the reads that outgrew the chain tier's.  What the wave form does not take (ambiguity codes in the
// read or its reference window, mates longer than 256 bases, overlapping mates, a structure that outgrows LDS) is left in c.todo for the
// lane-per-read passes.
static void runWaveForm(AlignCall& c, const bool tracePasses) {
  xm_index* idx = c.idx;
  const int64_t nq = c.nq;
  hipStream_t s = c.s;
  idx->wave.dListWaveHeavy.ensure((size_t)nq); idx->wave.dListWaveNext.ensure((size_t)nq); idx->wave.dListFallback.ensure((size_t)nq); idx->wave.dWaveCtl.ensure(1);
  idx->wave.dWaveSlotOf.ensure((size_t)nq);
  WaveCtl wctl{0, 0, 0, ~0ull};
  HIP_CHECK(hipMemcpyAsync(idx->wave.dWaveCtl.p, &wctl, sizeof(wctl), hipMemcpyHostToDevice, s));
  const OutView ov = idx->results.outView();
  const int lastTier = (int)envKnob("XM_WAVE_TIERS", 3, 1, 3) - 1;  // (experiment knob: 1 = light tier only, 2 = light + chain tier)
  int sWaves = 4, sLds = 1, sPerSimd = 4, memoBytes = 1, nodesPerWave = 1;
  xmSearchGeometry(&sWaves, &sLds, &sPerSimd, &memoBytes, &nodesPerWave);
  unsigned long long fallbackSoFar = 0;
  // one launch of a tier over `list` (null = all reads) + classification; returns the counts of the lists it filled
  auto launchTier = [&](int tier, const int64_t* list, long long n, int64_t* listNext, int32_t* slotOfOut, int64_t* listSearch) {
    WaveLaunch wl;
    wl.config = tier == 0 ? (idx->resident.anyPaired ? 1 : 0) : (tier == 1 ? (idx->resident.anyPaired ? 3 : 2) : 4);
    int wavesPerBlock = 1, ldsPerBlock = 1, wavesPerSimd = 1;
    xmWaveGeometry(wl.config, &wavesPerBlock, &ldsPerBlock, &wavesPerSimd);
    long long blocksPerCU = std::min<long long>((160 * 1024) / ldsPerBlock, (long long)(wavesPerSimd * 4) / wavesPerBlock);
    if (blocksPerCU < 1) blocksPerCU = 1;
    wl.itemsPerFetch = (int)envKnob(tier == 0 ? "XM_WAVE_FETCH" : "XM_WAVE_CHAIN_FETCH", tier == 0 ? 8 : 1, 1, 1024);
    long long blocks = std::min<long long>((long long)c.numCUs * blocksPerCU, (n + (long long)wavesPerBlock * wl.itemsPerFetch - 1) / ((long long)wavesPerBlock * wl.itemsPerFetch));
    if (blocks < 1) blocks = 1;
    wl.grid = (int)blocks; wl.block = wavesPerBlock * 64;
    wl.ix = c.view; wl.params = c.params; wl.batch = c.bv; wl.todo = list; wl.nTodo = n; wl.out = ov; wl.nextItem = idx->results.nextItem(); wl.counters = idx->passes.dCounters.p;
    wl.memoBase = (WMemo*)idx->wave.dWaveMemo.p; wl.slotOf = idx->wave.dWaveSlotOf.p;
    wl.waveNodes = nullptr;
    if (tier >= 1 && envInt("XM_WAVE_INLINE_SEARCH", 1) != 0) {  // (0: every search through the memo and the search kernel)
      idx->wave.dWaveNodes2.ensure(((size_t)blocks * wavesPerBlock * (size_t)xmWaveInlineNodeBytes() + sizeof(PNode) - 1) / sizeof(PNode));
      wl.waveNodes = idx->wave.dWaveNodes2.p;
    }
    HIP_CHECK(hipMemsetAsync(idx->results.nextItem(), 0, sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(idx->wave.dWaveCtl.p, 0, 2 * sizeof(unsigned long long), s));  // nNext, nSearch
    const float ms = timedLaunch(c, 1, tier == 0 ? 12 : 13, [&] {  // kernel microseconds: light tier / chain tiers
      const int rc = xmWaveLaunch(wl, (void*)s);
      if (rc != 0) throw std::runtime_error(std::string("wave kernel launch: ") + hipGetErrorString((hipError_t)rc));
    }, [&] {  // (the classification is not part of the tier's time)
      hipLaunchKernelGGL(xm_wave_classify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, list, n, idx->results.dStatus.p, listNext, slotOfOut, listSearch, idx->wave.dListFallback.p, idx->wave.dWaveCtl.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(&wctl, idx->wave.dWaveCtl.p, sizeof(wctl), hipMemcpyDeviceToHost, s));
      idx->results.readCursors(s);
    });
    if (tracePasses) fprintf(stderr, "[xm] wave tier %d config %d: reads %lld, %d x %d threads: %.3f ms -> next tier %llu, searches %llu, lane-per-read %llu (so far)\n", tier, wl.config, n, wl.grid,
                             wl.block, ms, listNext ? wctl.nNext : 0ull, wctl.nSearch, wctl.nFallback);
    if (wctl.errQuery != ~0ull) throwFailedQuery(idx->results.dStatus, wctl.errQuery);
    fallbackSoFar = wctl.nFallback;
  };
  auto launchSearches = [&](const int64_t* list, long long n) {
    SearchLaunch sl;
    long long blocks = std::min<long long>((long long)c.numCUs * std::min<long long>((160 * 1024) / sLds, (long long)(sPerSimd * 4) / sWaves), (n + sWaves - 1) / sWaves);
    if (blocks < 1) blocks = 1;
    sl.grid = (int)blocks; sl.block = sWaves * 64;
    sl.ix = c.view; sl.params = c.params; sl.batch = c.bv; sl.list = list; sl.n = n; sl.memoBase = (WMemo*)idx->wave.dWaveMemo.p; sl.slotOf = idx->wave.dWaveSlotOf.p; sl.nextItem = idx->results.nextItem();
    idx->wave.dWaveArenas.ensure((size_t)blocks * sWaves * (size_t)nodesPerWave);  // (node payloads: bytes per wave)
    sl.waveNodes = idx->wave.dWaveArenas.p; sl.counters = idx->passes.dCounters.p;
    HIP_CHECK(hipMemsetAsync(idx->results.nextItem(), 0, sizeof(unsigned long long), s));
    const float ms = timedLaunch(c, 1, 14, [&] {  // search kernel microseconds
      const int rc = xmSearchLaunch(sl, (void*)s);
      if (rc != 0) throw std::runtime_error(std::string("search kernel launch: ") + hipGetErrorString((hipError_t)rc));
    }, [] {});
    if (tracePasses) fprintf(stderr, "[xm] search kernel: %lld searches, %d x %d threads: %.3f ms\n", n, sl.grid, sl.block, ms);
  };
  // light tier
  launchTier(0, c.todo, c.nTodo, lastTier >= 1 ? idx->wave.dListWaveHeavy.p : (int64_t*)nullptr, idx->wave.dWaveSlotOf.p, nullptr);
  long long nChain = lastTier >= 1 ? (long long)wctl.nNext : 0;
  if (nChain > 0) {
    idx->wave.dWaveMemo.ensure((size_t)nChain * (size_t)memoBytes);
    if (xmMemoInitLaunch((WMemo*)idx->wave.dWaveMemo.p, nChain, (void*)s) != 0) throw std::runtime_error("memo init launch failed");
    idx->wave.dListWaveSearch[0].ensure((size_t)nChain); idx->wave.dListWaveSearch[1].ensure((size_t)nChain);
    long long nBig = 0;  // reads for the chain tier with the largest capacities (dListWaveNext, filled behind what is already there)
    for (int tier = 1; tier <= 2 && tier <= lastTier; tier++) {
      const int64_t* list = tier == 1 ? idx->wave.dListWaveHeavy.p : idx->wave.dListWaveNext.p;
      long long n = tier == 1 ? nChain : nBig;
      int which = 0, rounds = 0;
      while (n > 0) {
        // (tier 1 appends its hand-overs to dListWaveNext behind those of its earlier rounds)
        launchTier(tier, list, n, tier == 1 && lastTier >= 2 ? idx->wave.dListWaveNext.p + nBig : (int64_t*)nullptr, nullptr, idx->wave.dListWaveSearch[which].p);
        if (tier == 1 && lastTier >= 2) nBig += (long long)wctl.nNext;
        const long long nSearch = (long long)wctl.nSearch;
        if (nSearch == 0) break;
        if (++rounds > 4 * 16) throw std::runtime_error("internal error: search rounds do not end");
        launchSearches(idx->wave.dListWaveSearch[which].p, nSearch);
        list = idx->wave.dListWaveSearch[which].p; n = nSearch;
        which ^= 1;
      }
    }
  }
  c.todo = idx->wave.dListFallback.p;
  c.nTodo = (long long)fallbackSoFar;
  HIP_CHECK(hipMemsetAsync(idx->results.nextItem(), 0, sizeof(unsigned long long), s));
}

// scratch a context may hold now: up to its limit (halved `shift` times), never more than 3/4 of what is free (+ what this context already holds)
static unsigned long long scratchBudget(xm_index* idx, const BatchPolicy& pol, int shift) {
  unsigned long long want = pol.scratchWanted >> shift;
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
    const unsigned long long avail = (unsigned long long)(freeB + idx->passes.dArenas.n) / 4 * 3;
    if (want > avail) want = avail;
  }
  return want < (64ull << 20) ? (64ull << 20) : want;
}

// one launch of xm_align_kernel as planned, over c.todo; the control words and cursors it left are on the host when it returns
static float launchAlignPass(AlignCall& c, const BatchPolicy& pol, const PassState& st, const LaunchPlan& pl, PassCtl& ctl) {
  xm_index* idx = c.idx;
  PassBuffers& pb = idx->passes;
  ResultStage& rs = idx->results;
  hipStream_t s = c.s;
  pb.dWaveNodes.ensure((size_t)pl.grid * (pl.block / 64) * XM_PAL_NODES);
  AlignLaunch a{};
  a.grid = pl.grid; a.block = pl.block;
  a.launchConst = pb.launchConst(c.view, c.params, s); a.batch = c.bv;
  a.todo = c.todo; a.nTodo = c.nTodo;
  a.scale = st.scale; a.heavyAllowed = st.heavy ? 2 : (int)pol.k.lightLevel; a.lanesPerWave = pl.lpw;
  a.arenas = pb.dArenas.p + pl.regionsTotal; a.arenaBytes = (unsigned long long)pl.arenaBytes;
  a.out = rs.outView();
  a.nextItem = rs.nextItem(); a.counters = pb.dCounters.p;
  a.taperUnit = pl.taperUnit; a.firstStride = pl.firstStride;
  a.waveNodes = pb.dWaveNodes.p;
  a.ho = pb.handOver(pol, st, pl, rs.regionCursor()); a.pairLanes = pl.pairLanes; a.searchPool = pb.searchPool(st, pl);
  a.lists = pb.lists(st, c.nq, (int)pol.k.heavyHint);
  a.boundFilter = pl.boundFilterArg;
  HIP_CHECK(hipMemcpyAsync(rs.nextItem(), &pl.firstItem, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  return timedLaunch(c, 1, !st.heavy ? 12 : 15, [&] {  // kernel microseconds: light pass / gapped pass and reruns
    const int rc = xmAlignLaunch(a, (void*)s);
    if (rc != 0) throw std::runtime_error(std::string("align kernel launch: ") + hipGetErrorString((hipError_t)rc));
  }, [&] {
    HIP_CHECK(hipMemcpyAsync(&ctl, pb.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    rs.readCursors(s);
  });
}

// the lane-per-read passes over c.todo: plan -> allocate -> launch -> what follows (nextPass) -> take its list, until no list is left
static void runLanePasses(AlignCall& c, const BatchPolicy& pol) {
  xm_index* idx = c.idx;
  hipStream_t s = c.s;
  PassState st = firstPass(pol);
  int scratchShift = 0;  // the budget is halved after an allocation the GPU had no room for (another process, or contexts that were given more than there is)
  while (c.nTodo > 0) {
    LaunchPlan pl;
    {
      // contexts of one GPU size and allocate their scratch one after the other: they all look at the same free memory
      std::lock_guard<std::mutex> sizing(idx->dt->allocMu);
      pl = planLaunch(pol, st, c.nTodo, c.nq, c.numCUs, scratchBudget(idx, pol, scratchShift), idx->passes.dArenas.n);
      if (pl.scratchBytes > 0 && !idx->passes.dArenas.tryEnsure(pl.scratchBytes)) {  // (sized again with half the budget)
        if (++scratchShift > 8) throw std::runtime_error("no room in HBM for the scratch of even a few lanes (" + std::to_string(pl.scratchBytes >> 20) + " MiB asked)");
        continue;
      }
      if (st.hoMode == 1) {  // the pool's first regions are the lanes' own
        const unsigned long long firstFree = (unsigned long long)pl.lanes;
        HIP_CHECK(hipMemcpyAsync(idx->results.regionCursor(), &firstFree, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
      }
    }
    st.nRegions = pl.nRegions; st.regionsTotal = pl.regionsTotal;
    if (pl.boundFilter) c.boundFilterUsed = true;
    PassCtl ctl;
    const float ms = launchAlignPass(c, pol, st, pl, ctl);
#ifdef XM_LIGHT_ONLY
    fprintf(stderr, "[xm] light-only experiment build: pass %d %.3f ms\n", c.launches, ms);
    break;  // (experiment build, scripts/gpu_light_only.sh: only the first pass is meaningful)
#endif
    if (pol.k.tracePasses) fprintf(stderr, "[xm] pass %d: %s reads %lld scale %d lpw %d waves %lld lanes/read %d filter %d: %.3f ms -> heavy %llu scale %llu out %llu\n", c.launches,
                                   !st.heavy ? "light" : "gapped", c.nTodo, st.scale, pl.lpw, pl.nWaves, 1 << pl.pairLanes, pl.boundFilter, ms, ctl.nHeavy + ctl.nHeavyLate, ctl.nScale[st.ts], ctl.nOut[st.to]);
#ifdef XM_PROFILE
    if (pol.k.tracePasses && st.heavy) {  // reads of a wave that stood at a PathAligner call together, this pass
      unsigned long long a[16] = {0};
      HIP_CHECK((hipError_t)xmTakeArriveProf(a));
      fprintf(stderr, "[xm] pass %d: pair checks (status, result, search problem, search outcome): %llu %llu %llu %llu\n", c.launches, a[4], a[5], a[6], a[7]);
      fprintf(stderr, "[xm] pass %d: PathAligner arrivals %llu with %llu reads (%.2f per arrival); arrivals of four reads or more: %llu with %llu reads\n", c.launches, a[0], a[1], a[0] ? (double)a[1] / (double)a[0] : 0.0, a[2], a[3]);
    }
#endif
    if (ctl.errQuery != ~0ull) throwFailedQuery(idx->results.dStatus, ctl.errQuery);
    const NextPass np = nextPass(pol, st, ctl);
    c.nTodo = np.nTodo;
    if (np.kind == PassKind::Done) break;
    // what the next pass needs besides its list: room to spare in the result arenas; the values its reads waited for; (profile builds) the gapped pass's timers alone
    if (np.kind == PassKind::OutRerun) idx->results.growAfterOverflow(s);
    if (np.kind == PassKind::ConfRerun) { idx->conf.absorbMisses(s); idx->conf.fillView(c.view); }
#ifdef XM_HAVE_TICKS
    if (np.kind == PassKind::Gapped && pol.k.profGappedOnly) HIP_CHECK(hipMemsetAsync((char*)idx->passes.dCounters.p + offsetof(DevCounters, t), 0, sizeof(((DevCounters*)nullptr)->t), s));
#endif
    c.todo = idx->passes.take(np, ctl, s);
    if (np.kind != PassKind::Gapped) c.rerun += c.nTodo;
  }
}

// ---- canonical streams in query order (ResultStage::toHost) and the counters, timed between the context's events
static void finishStreams(AlignCall& c) {
  xm_index* idx = c.idx;
  xm_result* res = c.res;
  const int64_t nq = c.nq;
  hipStream_t s = c.s;
  float ms = 0;
  HIP_CHECK(hipEventRecord(idx->ev0, s));
#ifdef XM_READ_TIMES
  if (c.dReadTimes.p) {
    std::vector<unsigned long long> t((size_t)nq);
    HIP_CHECK(hipMemcpy(t.data(), c.dReadTimes.p, sizeof(unsigned long long) * (size_t)nq, hipMemcpyDeviceToHost));
    HIP_CHECK((hipError_t)xmSetReadTimes(nullptr));
    if (FILE* f = fopen(c.readTimesFile, "wb")) { fwrite(t.data(), sizeof(unsigned long long), t.size(), f); fclose(f); }
    c.dReadTimes.release();
  }
#endif
  idx->results.toHost(nq, c.copies, idx->residentGen, res, c.box, s, idx->resultCopy);
  DevCounters dc;
  HIP_CHECK(hipMemcpyAsync(&dc, idx->passes.dCounters.p, sizeof(dc), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipEventRecord(idx->ev1, s));
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipEventElapsedTime(&ms, idx->ev0, idx->ev1));
  res->d2h_ms = ms;
  if (idx->resultCopy) { res->num_ints = res->int_off[nq]; res->num_dbls = res->dbl_off[nq]; }  // (without the copy toHost read the two totals into them)
  countersToResult(dc, res);
  res->counters[11] = c.rerun;
  res->extra[3] = c.boundFilterUsed ? 1 : 0;
  res->extra[6] = c.remembered;
  res->extra[7] = c.copies;
#ifdef XM_HAVE_TICKS
  for (int i = 0; i < 16; i++) res->prof[i] = (int64_t)dc.t[i];
#else
  for (int i = 0; i < 16; i++) res->prof[i] = 0;  // (the phase timers exist in profile builds only)
#endif
  res->kernel_ms = c.kernelMs;
  res->kernel_launches = c.launches;
}

// ---- opening a context
// the caller's build options, or the defaults
static xm_build_opts buildOptsOrDefaults(const xm_build_opts* optsIn) {
  xm_build_opts o;
  memset(&o, 0, sizeof(o));
  o.enable_gapmers = 1; o.dup_window = 1000; o.dup_min_copies = 2; o.device = -1;
  if (optsIn) o = *optsIn;
  return o;
}
// the tables of hs in the HBM of `device`, uploaded: from the host, or with `peer` (the same tables on another GPU) from there (caller holds hs->mu where another context exists)
static std::shared_ptr<DeviceTables> makeDeviceTables(const std::shared_ptr<HostShare>& hs, int device, const DeviceTables* peer = nullptr) {
  auto dt = std::make_shared<DeviceTables>();
  dt->hs = hs; dt->device = device;
  std::unique_lock<std::shared_mutex> wr(dt->rw);
  dt->upload(peer);
  return dt;
}
// The first context of a new HostShare, for the entry named `entry`.  makeTables(host) fills the host tables - it builds them, or loads and completes them -
// with the GPU chosen and the device hasher in place (host_only: neither).
template <class MakeTables>
static int openFirstContext(const char* entry, const xm_build_opts& o, xm_index** out, MakeTables&& makeTables) {
  xm_index* idx = nullptr;
  try {
    idx = new xm_index();
    idx->hs = std::make_shared<HostShare>();
    idx->hostOnly = o.host_only != 0;
    if (!idx->hostOnly) {
      int n = 0;
      if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        throw std::runtime_error("no HIP device available: libxmapper_hip.so has no CPU path (pass host_only=1 only to inspect the index)");
      int dev = o.device;
      if (dev < 0) HIP_CHECK(hipGetDevice(&dev));
      idx->device = dev;
      idx->host().deviceHasher = &deviceHashLengths;  // the tables are hashed on this GPU (references without ambiguity codes)
      idx->host().deviceForBuild = dev;
    }
    makeTables(idx->host());
    idx->hs->hashedLength.store(idx->host().maxHashedLength);
    if (!idx->hostOnly) {
      idx->dt = makeDeviceTables(idx->hs, idx->device);
      idx->initContext();
    }
    *out = idx;
    return 0;
  } catch (std::exception& e) {
    delete idx;
    return fail(std::string(entry) + ": " + e.what());
  }
}

extern "C" {

const char* xm_last_error(void) { return g_error.c_str(); }
#ifndef XM_BUILD_STAMP
#define XM_BUILD_STAMP "unstamped"
#endif
const char* xm_build_stamp(void) { return XM_BUILD_STAMP; }
int32_t xm_abi_version(void) { return 12; }
int64_t xm_pinned_host_bytes(int64_t* high_water) {
  if (high_water) *high_water = (int64_t)g_pinned->highWater.load();
  return (int64_t)g_pinned->allocatedBytes.load();
}

int xm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int xm_index_build(const xm_ref* ref, const xm_build_opts* optsIn, xm_index** out) {
  if (!ref || !out) return fail("xm_index_build: null argument");
  const xm_build_opts o = buildOptsOrDefaults(optsIn);
  return openFirstContext("xm_index_build", o, out, [&](HostIndex& host) {
    host.setReference(ref->num_contigs, ref->names, ref->codes, ref->lengths);
    host.build(o.enable_gapmers, o.min_interesting_size, o.max_hashed_length, o.dup_window, o.dup_min_copies, o.dup_min_length, o.dup_max_length);
  });
}

int xm_index_replicate(xm_index* src, int32_t device, xm_index** out) {
  if (!src || !out) return fail("xm_index_replicate: null argument");
  if (src->hostOnly) return fail("xm_index_replicate: index was built with host_only=1");
  xm_index* idx = nullptr;
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("no HIP device available");
    if (device < 0 || device >= n) throw std::runtime_error("device " + std::to_string(device) + " does not exist (" + std::to_string(n) + " devices)");
    idx = new xm_index();
    idx->hs = src->hs;          // the host tables are shared, never copied
    idx->hostOnly = false;
    idx->device = device;
    idx->scratchBytes = src->scratchBytes;
    if (device == src->device) {
      idx->dt = src->dt;        // a context on the same GPU reads the same tables in HBM
    } else {
      int can = 0;
      HIP_CHECK(hipDeviceCanAccessPeer(&can, device, src->device));
      if (can) { HIP_CHECK(hipSetDevice(device)); hipError_t e = hipDeviceEnablePeerAccess(src->device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e); (void)hipGetLastError(); }
      std::lock_guard<std::mutex> lock(src->hs->mu);            // (not while the tables grow)
      std::shared_lock<std::shared_mutex> rd(src->dt->rw);      // (nor while the source's copy is brought up to them)
      // HBM to HBM (xGMI) where the source's copy is up to date
      idx->dt = makeDeviceTables(idx->hs, device, src->dt->uploadedLength == src->hs->host.maxHashedLength ? src->dt.get() : nullptr);
      HIP_CHECK(hipDeviceSynchronize());
    }
    idx->initContext();
    *out = idx;
    return 0;
  } catch (std::exception& e) {
    delete idx;
    return fail(std::string("xm_index_replicate: ") + e.what());
  }
}

int xm_context_new(xm_index* index, xm_index** out) {
  if (!index || !out) return fail("xm_context_new: null argument");
  return xm_index_replicate(index, index->device, out);
}

int xm_context_set_scratch(xm_index* idx, int64_t bytes) {
  if (!idx) return fail("xm_context_set_scratch: null argument");
  if (bytes < 0) return fail("xm_context_set_scratch: negative size");
  std::lock_guard<std::mutex> lock(idx->mu);
  idx->scratchBytes = bytes;
  if (bytes > 0 && idx->passes.dArenas.n > (size_t)bytes && !idx->hostOnly) {  // what the context holds beyond its new limit goes back to the GPU now
    (void)hipSetDevice(idx->device);
    idx->passes.dArenas.release();
  }
  return 0;
}

int xm_context_set_collapse(xm_index* idx, int32_t enable) {
  if (!idx) return fail("xm_context_set_collapse: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  idx->collapse = enable != 0;
  if (!idx->collapse && !idx->memoOn()) idx->collapseBufs = CollapseBuffers();
  return 0;
}

int xm_context_set_result_copy(xm_index* idx, int32_t on) {
  if (!idx) return fail("xm_context_set_result_copy: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  idx->resultCopy = on != 0;
  return 0;
}

// a memory of `generations` generations within max_bytes for the tables of `idx` on its GPU, emptied (the caller has set the device); -> null and *why
static std::shared_ptr<Memory> newMemory(xm_index* idx, int64_t max_bytes, int generations, bool isPrivate, std::string* why) {
  const MemoPlan plan = memoGenerationPlan(max_bytes, generations);
  if (generations < 1 || generations > XM_MEMO_MAX_GENERATIONS) { *why = "generations must be 1 or 2"; return nullptr; }
  if (plan.slots == 0) { *why = "the smallest memory is " + std::to_string(memoMinBytes(generations)) + " bytes" + (generations > 1 ? " (" + std::to_string(XM_MEMO_MIN_BYTES) + " per generation)" : ""); return nullptr; }
  auto m = std::make_shared<Memory>();
  m->device = idx->device; m->dt = idx->dt; m->hs = idx->hs; m->isPrivate = isPrivate;
  m->allocate(plan, generations);
  m->fingerprintBits = (int)envKnob("XM_MEMO_FINGERPRINT_BITS", 64, 1, 64);  // (test knob: fewer bits make different queries share a fingerprint)
  m->clear(idx->stream);
  HIP_CHECK(hipStreamSynchronize(idx->stream));
  return m;
}

int xm_context_set_memo(xm_index* idx, int64_t max_bytes) {
  if (!idx) return fail("xm_context_set_memo: null argument");
  if (max_bytes < 0) return fail("xm_context_set_memo: negative size");
  if (idx->hostOnly) return fail("xm_context_set_memo: index was built with host_only=1");
  const MemoPlan plan = memoPlan(max_bytes);
  if (max_bytes > 0 && plan.slots == 0) return fail("xm_context_set_memo: the smallest memory is " + std::to_string(XM_MEMO_MIN_BYTES) + " bytes");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->memo && !idx->memo->isPrivate) {
      if (max_bytes > 0) return fail("xm_context_set_memo: the context is attached to a shared memory (xm_context_attach_memory); detach it first");
      return 0;  // (no memory of its own to switch off)
    }
    HIP_CHECK(hipSetDevice(idx->device));
    HIP_CHECK(hipStreamSynchronize(idx->stream));
    idx->dropMemo();  // (what was remembered goes with the old budget)
    if (max_bytes == 0) {
      if (!idx->collapse) idx->collapseBufs = CollapseBuffers();
      return 0;
    }
    std::string why;
    std::shared_ptr<Memory> m = newMemory(idx, max_bytes, 1, true, &why);
    if (!m) return fail("xm_context_set_memo: " + why);
    m->timesEmptied = idx->memoEmptiedBefore;
    m->attached.fetch_add(1);
    idx->memo = m;
    return 0;
  } catch (std::exception& e) {
    return fail(std::string("xm_context_set_memo: ") + e.what());
  }
}

int xm_context_memo_info(xm_index* idx, int64_t out[4]) {
  if (!idx || !out) return fail("xm_context_memo_info: null argument");
  std::lock_guard<std::mutex> lock(idx->mu);
  const Memory* m = idx->memo && idx->memo->isPrivate ? idx->memo.get() : nullptr;
  out[0] = m ? (int64_t)memoRecordsHeld(m->gens) : 0;
  out[1] = m ? (int64_t)memoBytesInUse(m->plan, m->gens) : 0;
  out[2] = m ? (int64_t)m->plan.capacity : 0;
  out[3] = m ? m->timesEmptied : idx->memoEmptiedBefore;
  return 0;
}

// ---- the memory of a GPU: an object of its own that any number of the GPU's contexts of one index attach to
struct xm_memory {
  std::shared_ptr<Memory> m;
};

int xm_memory_new(xm_index* idx, int64_t max_bytes, int32_t generations, xm_memory** out) {
  if (!idx || !out) return fail("xm_memory_new: null argument");
  if (max_bytes < 0) return fail("xm_memory_new: negative size");
  if (idx->hostOnly) return fail("xm_memory_new: index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    HIP_CHECK(hipSetDevice(idx->device));
    std::string why;
    std::shared_ptr<Memory> m = newMemory(idx, max_bytes, (int)generations, false, &why);
    if (!m) return fail("xm_memory_new: " + why);
    *out = new xm_memory{m};
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_memory_new: ") + e.what()); }
}

int xm_context_attach_memory(xm_index* idx, xm_memory* memory) {
  if (!idx) return fail("xm_context_attach_memory: null argument");
  if (idx->hostOnly) return fail("xm_context_attach_memory: index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->memo && idx->memo->isPrivate) return fail("xm_context_attach_memory: the context has a memory of its own (xm_context_set_memo); switch it off first");
    if (memory) {
      if (memory->m->hs.lock() != idx->hs) return fail("xm_context_attach_memory: the memory belongs to another index (its records depend on the tables)");
      if (memory->m->device != idx->device || memory->m->dt.lock() != idx->dt)
        return fail("xm_context_attach_memory: the memory is on GPU " + std::to_string(memory->m->device) + ", the context on GPU " + std::to_string(idx->device));
      if (idx->memo == memory->m) return 0;
    }
    HIP_CHECK(hipSetDevice(idx->device));
    HIP_CHECK(hipStreamSynchronize(idx->stream));
    idx->dropMemo();
    if (memory) {
      memory->m->attached.fetch_add(1);
      idx->memo = memory->m;
    } else if (!idx->collapse) {
      idx->collapseBufs = CollapseBuffers();
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_context_attach_memory: ") + e.what()); }
}

int xm_memory_info(xm_memory* memory, int64_t out[8]) {
  if (!memory || !out) return fail("xm_memory_info: null argument");
  Memory& m = *memory->m;
  std::lock_guard<std::mutex> lock(m.mu);
  out[0] = (int64_t)memoRecordsHeld(m.gens);
  out[1] = (int64_t)memoBytesInUse(m.plan, m.gens);
  out[2] = (int64_t)m.plan.capacity * m.gens.generations;
  out[3] = m.timesEmptied;
  out[4] = m.gens.turns;
  out[5] = m.gens.promoted;
  out[6] = m.attached.load();
  out[7] = m.gens.generations;
  return 0;
}

void xm_memory_free(xm_memory* memory) { delete memory; }  // (the HBM goes with the last context that is attached, or now)

int xm_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes) {
  try {
    HIP_CHECK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIP_CHECK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_device_memory: ") + e.what()); }
}

int xm_index_save(xm_index* idx, const char* path) {
  if (!idx || !path) return fail("xm_index_save: null argument");
  try {
    std::lock_guard<std::mutex> lock(idx->hs->mu);
    idx->host().save(path);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_index_save: ") + e.what()); }
}

int xm_index_load(const char* path, const xm_ref* ref, const xm_build_opts* optsIn, xm_index** out) {
  if (!path || !out) return fail("xm_index_load: null argument");
  const xm_build_opts o = buildOptsOrDefaults(optsIn);
  return openFirstContext("xm_index_load", o, out, [&](HostIndex& host) {
    host.load(path);
    if (ref) {  // the file must answer exactly this build request (the reference's cache keys, M/HashBlock_Database.java:106-114)
      HostIndex want;
      want.setReference(ref->num_contigs, ref->names, ref->codes, ref->lengths);
      if (!host.matchesRequest(want, o.enable_gapmers, o.min_interesting_size, o.dup_window, o.dup_min_copies, o.dup_min_length, o.dup_max_length))
        throw std::runtime_error("the file was built from another reference or with other settings");
    }
    if (o.max_hashed_length > host.maxHashedLength) host.ensureLength(o.max_hashed_length);
  });
}

int xm_index_ensure_length(xm_index* idx, int32_t length) {
  if (!idx) return fail("null index");
  try {
    idx->ensureTablesFor(length);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_index_ensure_length: ") + e.what()); }
}

void xm_index_free(xm_index* idx) { delete idx; }

int xm_index_get_info(const xm_index* idx, xm_index_info_t* info) {
  if (!idx || !info) return fail("null argument");
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);  // (another context's batch may be growing the shared host tables)
  const HostIndex& h = idx->host();
  info->num_contigs = h.numContigs(); info->min_interesting_size = h.minInterestingSize; info->max_hashed_length = h.maxHashedLength;
  info->enable_gapmers = h.enableGapmers; info->dup_window = h.dupWindow; info->position_bytes = (idx->hostOnly ? h.seqCumStart.back() > 0xFFFFFFFFll : idx->dt->posIs64) ? 8 : 4;
  info->total_forward_size = h.totalForwardSize;
  info->num_positions = (int64_t)h.positions.size();
  info->index_bytes = (int64_t)(h.bucketOff.size() * 4 + h.positions.size() * (size_t)info->position_bytes + h.refCodes.size() + h.dupKeys.size() * 4);
  info->dup_granularity = h.dupGranularity();
  info->built_on_device = h.builtOnDevice ? 1 : 0;
  info->bucket_line_bytes = idx->hostOnly ? 0 : (idx->dt->view.lines64 ? 64 : (idx->dt->view.lines32 ? 32 : 0));
  info->hash_seconds = h.hashSeconds; info->duplication_seconds = h.dupSeconds;
  return 0;
}

int xm_index_table_info(const xm_index* idx, int32_t L, int32_t* capacity, int32_t* maxCount, int64_t* numStored, int64_t* numOverfull) {
  if (!idx) return fail("null index");
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);  // (another context's batch may be growing the shared host tables)
  const HostIndex& h = idx->host();
  if (L < 0 || L > h.maxHashedLength) return fail("length not hashed");
  const Table& t = h.tables[(size_t)L];
  *capacity = t.capacity; *maxCount = t.maxCount;
  int64_t o = 0;
  for (int k = 0; k < t.capacity; k++) if (h.bucketOff[(size_t)(t.offBase + k)] & XM_OVERFULL) o++;
  *numOverfull = o;
  *numStored = (int64_t)(h.bucketOff[(size_t)(t.offBase + t.capacity)] & ~XM_OVERFULL);
  return 0;
}

int xm_index_table_shape(const xm_index* idx, int32_t L, int32_t* capacity, int32_t* maxCount) {
  if (!idx || !capacity || !maxCount) return fail("null argument");
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);  // (another context's batch may be growing the shared host tables)
  const HostIndex& h = idx->host();
  if (L < 0 || L > h.maxHashedLength) return fail("length not hashed");
  *capacity = h.tables[(size_t)L].capacity; *maxCount = h.tables[(size_t)L].maxCount;
  return 0;
}

// How many buckets the hashed tables have, how many hold at least one position, and how many are overfull (more than max(L^2, 5) entries: dropped, HashBlock_Database.java:569-577)
int xm_index_bucket_stats(const xm_index* idx, int64_t* buckets, int64_t* occupied, int64_t* overfull) {
  if (!idx || !buckets || !occupied || !overfull) return fail("null argument");
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);
  const HostIndex& h = idx->host();
  int64_t nb = 0, no = 0, nf = 0;
  for (int L = 0; L <= h.maxHashedLength; L++) {
    const Table& t = h.tables[(size_t)L];
    if (t.capacity <= 1) continue;  // (the placeholder maps of lengths that are not hashed)
    nb += t.capacity;
    for (int k = 0; k < t.capacity; k++) {
      const uint32_t a = h.bucketOff[(size_t)t.offBase + (size_t)k], b = h.bucketOff[(size_t)t.offBase + (size_t)k + 1];
      if (a & XM_OVERFULL) nf++;
      else if ((b & ~XM_OVERFULL) > (a & ~XM_OVERFULL)) no++;
    }
  }
  *buckets = nb; *occupied = no; *overfull = nf;
  return 0;
}

int xm_index_table_dump(const xm_index* idx, int32_t L, int32_t* counts, int64_t* positionsOut) {
  if (!idx) return fail("null index");
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);  // (another context's batch may be growing the shared host tables)
  const HostIndex& h = idx->host();
  if (L < 0 || L > h.maxHashedLength) return fail("length not hashed");
  const Table& t = h.tables[(size_t)L];
  int64_t w = 0;
  for (int k = 0; k < t.capacity; k++) {
    uint32_t o0 = h.bucketOff[(size_t)(t.offBase + k)], o1 = h.bucketOff[(size_t)(t.offBase + k + 1)];
    if (o0 & XM_OVERFULL) { counts[k] = -1; continue; }
    int c = (int)((o1 & ~XM_OVERFULL) - (o0 & ~XM_OVERFULL));
    counts[k] = c;
    for (int j = 0; j < c; j++) positionsOut[w++] = (int64_t)h.positions[(size_t)(t.posBase + (o0 & ~XM_OVERFULL) + j)];
  }
  return 0;
}

int64_t xm_index_dup_keys(const xm_index* idx, int32_t contig, int32_t* out, int64_t cap) {
  if (!idx || contig < 0 || contig >= idx->host().numContigs()) return -1;
  std::lock_guard<std::mutex> hostLock(idx->hs->mu);  // (another context's batch may be growing the shared host tables)
  const HostIndex& h = idx->host();
  int64_t a = h.dupKeyStart[(size_t)contig], b = h.dupKeyStart[(size_t)contig + 1];
  for (int64_t i = a; i < b && i - a < cap; i++) out[i - a] = h.dupKeys[(size_t)i];
  return b - a;
}

void xm_result_free(xm_result* r) {
  if (!r) return;
  ResultBox* box = (ResultBox*)r;  // pub is the first member
  g_pinned->put(r->ints, box->bytesInts); g_pinned->put(r->dbls, box->bytesDbls);
  g_pinned->put(r->int_off, box->bytesIntOff); g_pinned->put(r->dbl_off, box->bytesDblOff);
  free(box);
}

// validation + Readable_HashBlock_Database growth + host-to-device copy of one batch; the batch stays resident in HBM
static int validateBatch(const xm_query_batch* b, bool* anyPaired = nullptr, std::vector<int32_t>* totalLengths = nullptr) {  // -> longest mate
  const int64_t nq = b->num_queries;
  int maxLen = 1;
  if (anyPaired) *anyPaired = false;
  std::vector<uint8_t> seen(totalLengths ? 60001 : 0, 0);   // total query lengths that occur (Query.getLength(): what the confidence table is keyed by)
  for (int64_t q = 0; q < nq; q++) {
    if (b->mate_count[q] < 1 || b->mate_count[q] > 2) throw std::runtime_error("mate_count must be 1 or 2");
    if (anyPaired && b->mate_count[q] == 2) *anyPaired = true;
    int total = 0;
    for (int m = 0; m < b->mate_count[q]; m++) {
      int32_t len = b->mate_length[q * 2 + m];
      if (len < 1 || len > 30000) throw std::runtime_error("mate length out of range (1..30000; longer reads are split by the caller as --split-queries-past-size does)");
      if (b->mate_offset[q * 2 + m] < 0 || b->mate_offset[q * 2 + m] + len > b->codes_length) throw std::runtime_error("mate outside of codes");
      if (len > maxLen) maxLen = len;
      total += len;
      if (totalLengths) seen[(size_t)len] = 1;
    }
    if (totalLengths) seen[(size_t)total] = 1;
  }
  if (totalLengths) {
    totalLengths->clear();
    for (size_t i = 0; i < seen.size(); i++) if (seen[i]) totalLengths->push_back((int32_t)i);
  }
  return maxLen;
}

static void uploadBatchLocked(xm_index* idx, const xm_query_batch* b) {
  DeviceBatch& d = idx->resident;
  bool anyPaired = false;
  const int maxLen = validateBatch(b, &anyPaired, &d.lens);
  d.anyPaired = anyPaired;
  idx->ensureTablesFor(maxLen);  // Readable_HashBlock_Database.getContainingMap growth, done before the launch
  HIP_CHECK(hipSetDevice(idx->device));
  d.copyIn(b, idx->ev0, idx->ev1, [&](auto&& queue) { queue(idx->stream); });
  idx->residentGen++;
  d.maxLen = maxLen;
}

static int alignResidentLocked(xm_index* idx, const xm_params* p, xm_result** out);

int xm_batch_upload(xm_index* idx, const xm_query_batch* b) {
  if (!idx || !b) return fail("xm_batch_upload: null argument");
  if (idx->hostOnly) return fail("xm_batch_upload: index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    uploadBatchLocked(idx, b);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_batch_upload: ") + e.what()); }
}

int xm_batch_stage(xm_index* idx, const xm_query_batch* b) {
  if (!idx || !b) return fail("xm_batch_stage: null argument");
  if (idx->hostOnly) return fail("xm_batch_stage: index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> stageLock(idx->stageMu);
    DeviceBatch& d = idx->staged;
    bool anyPaired = false;
    const int maxLen = validateBatch(b, &anyPaired, &d.lens);
    d.anyPaired = anyPaired;
    idx->ensureTablesFor(maxLen);  // (tables that grow wait for the launches that read them: DeviceTables::rw)
    HIP_CHECK(hipSetDevice(idx->device));
    if (!idx->cev0) { HIP_CHECK(hipEventCreate(&idx->cev0)); HIP_CHECK(hipEventCreate(&idx->cev1)); }
    d.copyIn(b, idx->cev0, idx->cev1, [&](auto&& queue) { idx->dt->onStagingStream(queue); });
    d.maxLen = maxLen;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_batch_stage: ") + e.what()); }
}

int xm_batch_commit(xm_index* idx) {
  if (!idx) return fail("xm_batch_commit: null argument");
  try {
    std::lock_guard<std::mutex> stageLock(idx->stageMu);
    if (idx->staged.nq < 0) return fail("xm_batch_commit: no staged batch (call xm_batch_stage first)");
    std::lock_guard<std::mutex> lock(idx->mu);  // (waits for a running xm_align_resident)
    std::swap(idx->resident, idx->staged);      // (the buffers of the batch before go on as the staging set)
    idx->staged.nq = -1;
    idx->residentGen++;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_batch_commit: ") + e.what()); }
}

int xm_batch_unstage(xm_index* idx) {
  if (!idx) return fail("xm_batch_unstage: null argument");
  try {
    std::lock_guard<std::mutex> stageLock(idx->stageMu);
    idx->staged.nq = -1;  // (its buffers stay: they are the staging set of the next xm_batch_stage)
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_batch_unstage: ") + e.what()); }
}

int xm_align_resident(xm_index* idx, const xm_params* p, xm_result** out) {
  if (!idx || !p || !out) return fail("xm_align_resident: null argument");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->resident.nq < 0) throw std::runtime_error("no batch is resident (call xm_batch_upload first)");
    return alignResidentLocked(idx, p, out);
  } catch (std::exception& e) { return fail(std::string("xm_align_resident: ") + e.what()); }
}

int xm_align_batch(xm_index* idx, const xm_params* p, const xm_query_batch* b, xm_result** out) {
  if (!idx || !p || !b || !out) return fail("xm_align_batch: null argument");
  if (idx->hostOnly) return fail("xm_align_batch: index was built with host_only=1; this library aligns on the GPU only");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    uploadBatchLocked(idx, b);
    int rc = alignResidentLocked(idx, p, out);
    if (rc == 0) (*out)->h2d_ms = idx->resident.h2dMs;
    return rc;
  } catch (std::exception& e) {
    return fail(std::string("xm_align_batch: ") + e.what());
  }
}

static int alignResidentLocked(xm_index* idx, const xm_params* p, xm_result** out) {
  ResultBox* box = (ResultBox*)calloc(1, sizeof(ResultBox));
  xm_result* res = &box->pub;
  try {
    const int64_t nq = idx->resident.nq;
    idx->results.forgetLast();
    HIP_CHECK(hipSetDevice(idx->device));
    // the shared tables stay as they are while this call's kernels read them (another context that grows them waits; so does this one's next growth)
    std::shared_lock<std::shared_mutex> tablesInUse(idx->dt->rw);
    res->num_queries = nq;
    if (idx->resultCopy) {  // (xm_context_set_result_copy(0): the result has no streams, and no pinned buffer is taken for one)
      res->int_off = (int64_t*)g_pinned->get(sizeof(int64_t) * (size_t)(nq + 1), &box->bytesIntOff);
      res->dbl_off = (int64_t*)g_pinned->get(sizeof(int64_t) * (size_t)(nq + 1), &box->bytesDblOff);
    }
    if (nq == 0) {
      if (idx->resultCopy) {
        res->ints = (int32_t*)g_pinned->get(4, &box->bytesInts); res->dbls = (double*)g_pinned->get(8, &box->bytesDbls);
        res->int_off[0] = res->dbl_off[0] = 0;
      }
      *out = res;
      return 0;
    }
    AlignCall c;
    c.idx = idx; c.box = box; c.res = res; c.nq = nq; c.s = idx->stream; c.numCUs = idx->dt->numCUs;
    c.view = idx->dt->view;
    c.params = paramsFromC(*p);
    c.cParams = *p;
    c.bv = idx->resident.view();
    prepareCall(c);
    if (idx->collapse || idx->memoOn()) collapseBuildList(c);  // (a run-wide memory includes the batch)
    std::unique_lock<std::mutex> memoInUse;  // (a): from before the lookup until replay and promotion have completed on the stream
    if (idx->memoOn()) {
      // The result arenas are sized between lookup and replay, inside (a) - but they never GROW there: a buffer that grows is freed first, and that waits for
      // the whole device, the other contexts' running passes included, while their lookups and inserts would be locked out.  A call whose hits need more room
      // than the arenas have lets go of the memory, grows them (with an eighth to spare) and looks everything up again: the memory may have changed meanwhile.
      const long long nReps = c.nTodo;
      for (;;) {
        memoInUse = memoLock(c);
        c.nTodo = nReps;
        memoLookup(c);
        if (idx->results.arenasHold(nq, c.hitInts, c.hitDbls)) break;
        memoInUse.unlock();
        idx->results.reserveArenas(nq, c.hitInts, c.hitDbls, true);
      }
    }
    const BatchFacts facts{idx->resident.maxLen, idx->resident.anyPaired, idx->dt->contexts.load(), idx->scratchBytes};
    const BatchPolicy pol = makePolicy(facts, readPassKnobs(facts));
    idx->results.reserveArenas(nq, c.hitInts, c.hitDbls);  // (the remembered results on top; with a memory: there already)
    if (c.remembered > 0) memoReplay(c);
    if (idx->memoOn()) { memoPromote(c); memoInUse.unlock(); }
    if (pol.k.handOver) idx->passes.forgetRegions(nq, c.s);
    if (pol.k.waveForm && idx->resident.maxLen <= 256 && c.nTodo > 0) runWaveForm(c, pol.k.tracePasses);
    runLanePasses(c, pol);  // (nothing left to align: no pass runs)
    if (idx->memoOn()) { memoInsert(c); res->reserved = (int32_t)std::min<double>(c.memoWaitUs, 2147483647.0); }  // (b), under the memory's mu
    if (c.copies > 0) collapseFanOut(c);
    finishStreams(c);
    *out = res;
    return 0;
  } catch (...) {
    xm_result_free(res);
    throw;
  }
}

}  // extern "C"

#include "xm_capi_probe.h"
#include "xm_capi_pileup.h"
#include "xm_capi_mutations.h"
#include "xm_capi_sam.h"
#include "xm_capi_summary.h"
#include "xm_capi_refs.h"
#include "xm_capi_unaligned.h"
#include "xm_capi_test.h"
#include "xm_capi_fastq.h"
#include "xm_capi_fasta.h"
