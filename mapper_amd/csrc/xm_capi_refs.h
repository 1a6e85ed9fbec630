// xm_refs_count_last, xm_refs_count_free (included once, by xm_capi.hip): the queries of the last align call counted per combination of contigs - the
// count behind --out-refs-map-count - by the kernels of xm_refs.h from the streams where they lie in HBM - xm_summary_last's contract (the context's mutex and
// stream, ResultStage::lastStreams) - and the records copied to pinned buffers of the library's pool.  refsRun is the part that xm_test_refs_count runs over
// host-given arrays as well.
#pragma once
#include "xm_refs.h"

namespace {

// xm_refs_count plus what xm_refs_count_free needs to know about its buffers
struct RefsBox {
  xm_refs_count pub;
  size_t bytesRecords, bytesOffsets, bytesContigs;
};

void freeRefsBox(RefsBox* box) {
  g_pinned->put(box->pub.records, box->bytesRecords);
  g_pinned->put(box->pub.leftover_offsets, box->bytesOffsets);
  g_pinned->put(box->pub.leftover_contigs, box->bytesContigs);
  free(box);
}

// The four stages on stream s over streams in HBM; bits: what refsFingerprint keeps (64 outside of tests).  Returns the count, its arrays in pinned buffers
// (NULL where there is nothing to hold), or throws: a malformed slice gives no count.
RefsBox* refsRun(RefsStage& g, const xm::ResultStreams& st, int64_t nq, int bits, hipStream_t s) {
  RefsBox* box = (RefsBox*)calloc(1, sizeof(RefsBox));
  if (!box) throw std::runtime_error("out of host memory");
  box->pub.store = box;
  box->pub.num_queries = nq;
  if (nq == 0) return box;  // (nothing is launched)
  try {
    if (nq > (1ll << 30)) throw std::runtime_error("more than 2^30 queries");  // (a slot is an int32)
    g.ev.ready();
    // everything that is sized by the queries (a buffer that grows frees the old one, which waits for the device: before anything is queued)
    size_t cap = 2;
    while (cap < 2 * (size_t)nq) cap <<= 1;
    g.dKeys.ensure(cap); g.dReps.ensure(cap); g.dCounts.ensure(cap);
    g.dSlotOf.ensure((size_t)nq); g.dLeftLen.ensure((size_t)nq); g.dLeftFlag.ensure((size_t)nq); g.dIsRep.ensure((size_t)nq);
    g.dOff.ensure((size_t)nq + 1); g.dLoff.ensure((size_t)nq + 1); g.dLqoff.ensure((size_t)nq + 1);
    g.dBlockSums.ensure(xmScanSums(nq, 3)); g.dCtl.ensure(XM_REFS_CTL_WORDS);
    const RefsTable table{g.dKeys.p, g.dReps.p, g.dCounts.p, (unsigned long long)cap - 1};
    const unsigned grid = (unsigned)((nq + 255) / 256);
    HIP_CHECK(hipEventRecord(g.ev[0], s));
    HIP_CHECK(hipMemsetAsync(g.dCtl.p, 0xFF, sizeof(unsigned long long), s));      // XM_NO_QUERY
    HIP_CHECK(hipMemsetAsync(g.dCtl.p + 1, 0, sizeof(unsigned long long), s));     // aligned queries
    HIP_CHECK(hipMemsetAsync(g.dKeys.p, 0, sizeof(unsigned long long) * cap, s));
    HIP_CHECK(hipMemsetAsync(g.dCounts.p, 0, sizeof(unsigned long long) * cap, s));
    HIP_CHECK(hipMemsetAsync(g.dReps.p, 0xFF, sizeof(unsigned long long) * cap, s));  // XM_REFS_NO_REP
    hipLaunchKernelGGL(xm_refs_claim_kernel, dim3(grid), dim3(256), 0, s, st, (long long)nq, bits, table, g.dSlotOf.p, g.dLeftLen.p, g.dLeftFlag.p, g.dCtl.p);
    hipLaunchKernelGGL(xm_refs_verify_kernel, dim3(grid), dim3(256), 0, s, st, (long long)nq, table, g.dSlotOf.p, g.dLeftLen.p, g.dLeftFlag.p, g.dIsRep.p);
    xmScan(XmOffsets<int32_t, 3>{nq, {g.dIsRep.p, g.dLeftLen.p, g.dLeftFlag.p}, {g.dOff.p, g.dLoff.p, g.dLqoff.p}}, nq, g.dBlockSums, s);
    HIP_CHECK(hipEventRecord(g.ev[1], s));
    unsigned long long ctl[XM_REFS_CTL_WORDS] = {0, 0};
    int64_t totals[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[0], g.dOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[1], g.dLoff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[2], g.dLqoff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the one wait for the control word and the totals)
    throwIfMalformed(ctl[0]);
    const size_t nRec = (size_t)totals[0], nLeft = (size_t)totals[1], nLeftQ = (size_t)totals[2];
    box->pub.num_aligned = (int64_t)ctl[1];
    box->pub.num_combinations = (int64_t)nRec; box->pub.num_leftover_queries = (int64_t)nLeftQ;
    if (nRec) { g.dRecords.ensure(nRec); box->pub.records = (xm_refs_record*)g_pinned->get(sizeof(xm_refs_record) * nRec, &box->bytesRecords); }
    if (nLeftQ) {
      g.dLeft.ensure(nLeft); g.dLeftStart.ensure(nLeftQ);
      box->pub.leftover_offsets = (int64_t*)g_pinned->get(sizeof(int64_t) * (nLeftQ + 1), &box->bytesOffsets);
      box->pub.leftover_contigs = (int32_t*)g_pinned->get(sizeof(int32_t) * (nLeft ? nLeft : 1), &box->bytesContigs);
    }
    HIP_CHECK(hipEventRecord(g.ev[2], s));
    if (nRec || nLeftQ) {
      // (a record or a start that no lane writes - the second walk of a slice can only differ from the first if the streams changed - must not be garbage)
      if (nRec) HIP_CHECK(hipMemsetAsync(g.dRecords.p, 0, sizeof(RefsRecord) * nRec, s));
      if (nLeftQ) HIP_CHECK(hipMemsetAsync(g.dLeftStart.p, 0, sizeof(int64_t) * nLeftQ, s));
      if (nLeft) HIP_CHECK(hipMemsetAsync(g.dLeft.p, 0, sizeof(int32_t) * nLeft, s));
      hipLaunchKernelGGL(xm_refs_gather_kernel, dim3(grid), dim3(256), 0, s, st, (long long)nq, table, (const int32_t*)g.dSlotOf.p, (const int64_t*)g.dOff.p, (const int64_t*)g.dLoff.p,
                         (const int64_t*)g.dLqoff.p, nRec ? g.dRecords.p : nullptr, (long long)nRec, nLeft ? g.dLeft.p : nullptr, (long long)nLeft,
                         nLeftQ ? g.dLeftStart.p : nullptr, (long long)nLeftQ);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(g.ev[3], s));
    if (nRec) HIP_CHECK(hipMemcpyAsync(box->pub.records, g.dRecords.p, sizeof(RefsRecord) * nRec, hipMemcpyDeviceToHost, s));
    if (nLeftQ) HIP_CHECK(hipMemcpyAsync(box->pub.leftover_offsets, g.dLeftStart.p, sizeof(int64_t) * nLeftQ, hipMemcpyDeviceToHost, s));
    if (nLeft) HIP_CHECK(hipMemcpyAsync(box->pub.leftover_contigs, g.dLeft.p, sizeof(int32_t) * nLeft, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(g.ev[4], s));
    HIP_CHECK(hipEventSynchronize(g.ev[4]));
    if (nLeftQ) box->pub.leftover_offsets[nLeftQ] = (int64_t)nLeft;
    float count = 0, gather = 0, down = 0;
    HIP_CHECK(hipEventElapsedTime(&count, g.ev[0], g.ev[1]));
    HIP_CHECK(hipEventElapsedTime(&gather, g.ev[2], g.ev[3]));
    HIP_CHECK(hipEventElapsedTime(&down, g.ev[3], g.ev[4]));
    box->pub.kernel_ms = (double)count + gather; box->pub.d2h_ms = down;
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // (nothing of this call is still in flight when its buffers go)
    freeRefsBox(box);
    throw;
  }
}

}  // namespace

extern "C" {

void xm_refs_count_free(xm_refs_count* count) {
  if (count) freeRefsBox((RefsBox*)count);  // pub is the first member
}

int xm_refs_count_last(xm_index* idx, xm_refs_count** out) {
  return lastCallEntry(idx, out, "xm_refs_count_last", [&] {
    const ResultStage::LastStreams last = lastCall(idx, "xm_refs_count_last");
    return &refsRun(idx->refs, last.streams(idx->host().numContigs()), last.nq, 64, idx->stream)->pub;
  });
}

}  // extern "C"
