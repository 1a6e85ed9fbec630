// The result stage of a context (included once, by xm_capi.hip, behind xm_scan.h, xm_pass_plan.h and its `using namespace xm`): where the passes
// of an align call leave their results and how those become the streams the caller gets.  Every kernel that publishes a read writes its slice into one of two arenas through the call's
// cursors and notes offset, length and status per query (OutView, xm_kernel_args.h); after the last pass the lengths are prefix-summed in query order (xm_scan.h), the
// slices gathered into canonical streams on the device, and the streams copied to pinned host memory.  The arenas are per context and only ever grow: how
// large they start and what an overflow grows them to is xm_pass_plan.h (firstArenaSize, grownArenaSize).  The canonical streams stay in HBM until the
// next call (xm_pileup_add_last reads them there: lastStreams).
#pragma once

namespace {

// canonical streams: every query's slice copied from where its pass left it to its place in query order
__global__ void __launch_bounds__(256) xm_gather_kernel(long long nq, const int64_t* srcIntOff, const int64_t* srcDblOff, const int32_t* intLen, const int32_t* dblLen,
                                                        const int64_t* finalIntOff, const int64_t* finalDblOff, const int32_t* srcInts, const double* srcDbls,
                                                        int32_t* dstInts, double* dstDbls) {
  long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int32_t* si = srcInts + srcIntOff[q]; int32_t* di = dstInts + finalIntOff[q];
  const double* sd = srcDbls + srcDblOff[q]; double* dd = dstDbls + finalDblOff[q];
  int ni = intLen[q], nd = dblLen[q];
  for (int k = 0; k < ni; k++) di[k] = si[k];
  for (int k = 0; k < nd; k++) dd[k] = sd[k];
}

struct ResultStage {
  DevBuf<int32_t> dOutInts;                       // the two arenas
  DevBuf<double> dOutDbls;
  DevBuf<unsigned long long> dCursors;            // [0],[1] what is used of them; [2] the next item of a launch's work list, [3] the next unused hand-over region
  DevBuf<int32_t> dStatus, dIntLen, dDblLen;      // per query: status, and where its slices are
  DevBuf<int64_t> dIntOff, dDblOff;
  DevBuf<long long> dBlockSums;                   // the scan's block sums
  DevBuf<int64_t> dFinalIntOff, dFinalDblOff;     // [nq + 1] the canonical streams: offsets ...
  DevBuf<int32_t> dFinalInts;                     // ... and slices in query order
  DevBuf<double> dFinalDbls;
  int64_t lastAlignedNq = -1, lastAlignedGen = -1;  // queries whose canonical streams are still in HBM from the last align call, and the resident batch they belong to
  unsigned long long cursors[4] = {0, 0, 0, 0};   // the host's copy of dCursors after the last launch that read it back (readCursors)

  // sized and cleared for a call of nq queries (the arenas: reserveArenas)
  void prepare(int64_t nq, hipStream_t s) {
    dStatus.ensure((size_t)nq); dIntOff.ensure((size_t)nq); dDblOff.ensure((size_t)nq); dIntLen.ensure((size_t)nq); dDblLen.ensure((size_t)nq);
    dCursors.ensure(4);
    HIP_CHECK(hipMemsetAsync(dCursors.p, 0, sizeof(unsigned long long) * 4, s));
    for (unsigned long long& v : cursors) v = 0;
  }
  // the arenas hold at least the first size for nq queries plus the slices of the hits of a memory (their ints, their doubles) ...
  bool arenasHold(int64_t nq, unsigned long long hitInts, unsigned long long hitDbls) const {
    return dOutInts.p && dOutInts.n >= firstArenaSize(nq, hitInts, false) && dOutDbls.p && dOutDbls.n >= firstArenaSize(nq, hitDbls, true);
  }
  // ... and are made to (a buffer that grows is freed first, and that waits for the whole device); spareEighth: with an eighth of the hits on top
  void reserveArenas(int64_t nq, unsigned long long hitInts, unsigned long long hitDbls, bool spareEighth = false) {
    dOutInts.ensure(firstArenaSize(nq, hitInts, false) + (spareEighth ? (size_t)hitInts / 8 : 0));
    dOutDbls.ensure(firstArenaSize(nq, hitDbls, true) + (spareEighth ? (size_t)hitDbls / 8 : 0));
  }
  OutView outView() const { return OutView{dOutInts.p, dOutDbls.p, dOutInts.n, dOutDbls.n, dCursors.p, dStatus.p, dIntOff.p, dDblOff.p, dIntLen.p, dDblLen.p}; }
  unsigned long long* nextItem() const { return dCursors.p + 2; }
  unsigned long long* regionCursor() const { return dCursors.p + 3; }
  void readCursors(hipStream_t s) { HIP_CHECK(hipMemcpyAsync(cursors, dCursors.p, sizeof(cursors), hipMemcpyDeviceToHost, s)); }  // (enqueued: the caller waits for s)
  // after a pass that found an arena full (PassKind::OutRerun): both grow, and keep what the cursors say is used
  void growAfterOverflow(hipStream_t s) {
    const unsigned long long intCap = dOutInts.n, dblCap = dOutDbls.n;
    dOutInts.growKeep((size_t)grownArenaSize(intCap, cursors[0]), (size_t)std::min(cursors[0], intCap), s);
    dOutDbls.growKeep((size_t)grownArenaSize(dblCap, cursors[1]), (size_t)std::min(cursors[1], dblCap), s);
  }
  // Canonical streams in query order: offsets by prefix sum, slices gathered on the device, one copy per stream to pinned host memory (enqueued on s: the
  // caller waits for it).  copies: queries that share their representative's slice (collapseFanOut); gen: the resident batch these streams belong to.
  // copy = false (xm_context_set_result_copy(0)): the same launches, the streams stay where they lie, and only the scan's two totals are read, into res->num_ints / num_dbls.
  void toHost(int64_t nq, int64_t copies, int64_t gen, xm_result* res, ResultBox* box, hipStream_t s, bool copy = true) {
    dBlockSums.ensure(xmScanSums(nq, 2));
    dFinalIntOff.ensure((size_t)nq + 1); dFinalDblOff.ensure((size_t)nq + 1);
    size_t usedI = (size_t)std::min<unsigned long long>(cursors[0], dOutInts.n), usedD = (size_t)std::min<unsigned long long>(cursors[1], dOutDbls.n);  // upper bounds of the totals
    if (copies == 0) { dFinalInts.ensure(usedI); dFinalDbls.ensure(usedD); }
    const XmOffsets<int32_t, 2> lengths{nq, {dIntLen.p, dDblLen.p}, {dFinalIntOff.p, dFinalDblOff.p}};
    xmScanTotals(lengths, nq, dBlockSums, s);
    if (copies > 0) {  // (a copy's slice is in the result arena once and in the streams once per copy: the totals are the scan's)
      int64_t totals[2] = {0, 0};
      HIP_CHECK(hipMemcpyAsync(&totals[0], dFinalIntOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&totals[1], dFinalDblOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      usedI = (size_t)totals[0]; usedD = (size_t)totals[1];
      dFinalInts.ensure(usedI); dFinalDbls.ensure(usedD);
    }
    xmScanPlace(lengths, nq, dBlockSums, s);
    hipLaunchKernelGGL(xm_gather_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (long long)nq, dIntOff.p, dDblOff.p, dIntLen.p, dDblLen.p,
                       dFinalIntOff.p, dFinalDblOff.p, dOutInts.p, dOutDbls.p, dFinalInts.p, dFinalDbls.p);
    HIP_CHECK(hipGetLastError());
    if (!copy) {
      lastAlignedNq = nq;
      lastAlignedGen = gen;
      HIP_CHECK(hipMemcpyAsync(&res->num_ints, dFinalIntOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&res->num_dbls, dFinalDblOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      return;
    }
    res->ints = (int32_t*)g_pinned->get(sizeof(int32_t) * (usedI ? usedI : 1), &box->bytesInts);
    res->dbls = (double*)g_pinned->get(sizeof(double) * (usedD ? usedD : 1), &box->bytesDbls);
    lastAlignedNq = nq;
    lastAlignedGen = gen;
    HIP_CHECK(hipMemcpyAsync(res->int_off, dFinalIntOff.p, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(res->dbl_off, dFinalDblOff.p, sizeof(int64_t) * (size_t)(nq + 1), hipMemcpyDeviceToHost, s));
    if (usedI) HIP_CHECK(hipMemcpyAsync(res->ints, dFinalInts.p, sizeof(int32_t) * usedI, hipMemcpyDeviceToHost, s));
    if (usedD) HIP_CHECK(hipMemcpyAsync(res->dbls, dFinalDbls.p, sizeof(double) * usedD, hipMemcpyDeviceToHost, s));
  }
  // an align call begins: until it has succeeded (toHost) there are no streams of a last call - a call that fails leaves none behind
  void forgetLast() { lastAlignedNq = -1; lastAlignedGen = -1; }
  // the streams of the last call where they lie in HBM, if they belong to the resident batch of generation gen with nq queries (else: nq = -1)
  struct LastStreams {
    int64_t nq; const int32_t* ints; const int64_t* intOff; size_t intsHeld; const double* dbls; const int64_t* dblOff;
    // as the walk of a slice takes them (xm_result_walk.h), for an index of numContigs contigs
    ResultStreams streams(int64_t numContigs) const { return ResultStreams{ints, dbls, intOff, dblOff, (int32_t)numContigs}; }
  };
  LastStreams lastStreams(int64_t gen, int64_t nq) const {
    if (lastAlignedNq < 0 || lastAlignedNq != nq || lastAlignedGen != gen) return LastStreams{-1, nullptr, nullptr, 0, nullptr, nullptr};
    return LastStreams{lastAlignedNq, dFinalInts.p, dFinalIntOff.p, dFinalInts.n, dFinalDbls.p, dFinalDblOff.p};
  }
};

// The error of a call whose pass left an error status for `query`.
[[noreturn]] void throwFailedQuery(const DevBuf<int32_t>& status, unsigned long long query) {
  int32_t code = 0;
  HIP_CHECK(hipMemcpy(&code, status.p + query, sizeof(code), hipMemcpyDeviceToHost));
  code &= 0xFF;
  if (code == XM_ST_NEED_GROW) throw std::runtime_error("Failed to align query " + std::to_string(query) + ": gapmer longer than the hashed lengths");
  throw std::runtime_error("Failed to align query " + std::to_string(query) + ": the reference implementation would have thrown here (status " + std::to_string(code) + ")");
}

// The error of a stage whose walk (xm_result_walk.h) left `query` as the lowest one with a malformed slice; nothing to do while there is none.
void throwIfMalformed(unsigned long long query) {
  if (query != XM_NO_QUERY) throw std::runtime_error("malformed result streams: query " + std::to_string(query));
}

}  // namespace
