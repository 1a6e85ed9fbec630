// xm_summary_last, xm_summary_free (included once, by xm_capi.hip): what the host still needs of the last align call's result streams when the SAM text is
// made on the GPU - the four statistics, every alignment's penalty in stream order and the list of unaligned queries - computed by the kernels of xm_summary.h
// from the streams where they lie in HBM - xm_pileup_add_last's contract (the context's mutex and stream, ResultStage::lastStreams) - and copied to pinned
// buffers of the library's pool.  With xm_context_set_result_copy(0) these few bytes and the SAM text are all that crosses to the host of a batch's results.
// summaryRun is the part that xm_test_summary runs over host-given arrays as well.
#pragma once
#include "xm_summary.h"

namespace {

// xm_batch_summary plus what xm_summary_free needs to know about its buffers
struct SummaryBox {
  xm_batch_summary pub;
  size_t bytesPenalties, bytesUnaligned;
};

void freeSummaryBox(SummaryBox* box) {
  g_pinned->put(box->pub.penalties, box->bytesPenalties);
  g_pinned->put(box->pub.unaligned, box->bytesUnaligned);
  free(box);
}

// The three stages on stream s over streams in HBM.  Returns the summary, its two arrays in pinned buffers (NULL where there is nothing to hold), or throws:
// a malformed slice gives no summary.
SummaryBox* summaryRun(SummaryStage& g, const xm::ResultStreams& st, int64_t nq, bool wantUnaligned, hipStream_t s) {
  SummaryBox* box = (SummaryBox*)calloc(1, sizeof(SummaryBox));
  if (!box) throw std::runtime_error("out of host memory");
  box->pub.store = box;
  box->pub.num_queries = nq;
  if (nq == 0) return box;  // (nothing is launched)
  try {
    g.ev.ready();
    // everything that is sized by the queries (a buffer that grows frees the old one, which waits for the device: before anything is queued)
    g.dAlignments.ensure((size_t)nq); g.dUnalignedFlag.ensure((size_t)nq); g.dOff.ensure((size_t)nq + 1); g.dUoff.ensure((size_t)nq + 1);
    g.dBlockSums.ensure(xmScanSums(nq, 2)); g.dCtl.ensure(XM_SUMMARY_CTL_WORDS);
    const unsigned grid = (unsigned)((nq + 255) / 256);
    HIP_CHECK(hipEventRecord(g.ev[0], s));
    HIP_CHECK(hipMemsetAsync(g.dCtl.p, 0xFF, sizeof(unsigned long long), s));                                               // XM_NO_QUERY
    HIP_CHECK(hipMemsetAsync(g.dCtl.p + 1, 0, sizeof(unsigned long long) * (XM_SUMMARY_CTL_WORDS - 1), s));                 // the three counters
    hipLaunchKernelGGL(xm_summary_measure_kernel, dim3(grid), dim3(256), 0, s, st, (long long)nq, g.dAlignments.p, g.dUnalignedFlag.p, g.dCtl.p);
    xmScan(XmOffsets<int32_t, 2>{nq, {g.dAlignments.p, g.dUnalignedFlag.p}, {g.dOff.p, g.dUoff.p}}, nq, g.dBlockSums, s);
    HIP_CHECK(hipEventRecord(g.ev[1], s));
    unsigned long long ctl[XM_SUMMARY_CTL_WORDS] = {0, 0, 0, 0};
    int64_t totals[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[0], g.dOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[1], g.dUoff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the one wait for the totals and the counters)
    throwIfMalformed(ctl[0]);
    const size_t nAl = (size_t)totals[0], nUn = wantUnaligned ? (size_t)totals[1] : 0;
    box->pub.num_aligned = (int64_t)ctl[1]; box->pub.total_aligned_length = (int64_t)ctl[2]; box->pub.num_indels = (int64_t)ctl[3];
    box->pub.num_alignments = (int64_t)nAl; box->pub.num_unaligned = (int64_t)nUn;
    if (nAl) { g.dPenalties.ensure(nAl); box->pub.penalties = (double*)g_pinned->get(sizeof(double) * nAl, &box->bytesPenalties); }
    if (nUn) { g.dUnaligned.ensure(nUn); box->pub.unaligned = (int64_t*)g_pinned->get(sizeof(int64_t) * nUn, &box->bytesUnaligned); }
    HIP_CHECK(hipEventRecord(g.ev[2], s));
    if (nAl || nUn) {
      hipLaunchKernelGGL(xm_summary_gather_kernel, dim3(grid), dim3(256), 0, s, st, (long long)nq, (const int64_t*)g.dOff.p, (const int64_t*)g.dUoff.p,
                         nAl ? g.dPenalties.p : nullptr, (long long)nAl, nUn ? g.dUnaligned.p : nullptr, (long long)nUn);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(g.ev[3], s));
    if (nAl) HIP_CHECK(hipMemcpyAsync(box->pub.penalties, g.dPenalties.p, sizeof(double) * nAl, hipMemcpyDeviceToHost, s));
    if (nUn) HIP_CHECK(hipMemcpyAsync(box->pub.unaligned, g.dUnaligned.p, sizeof(int64_t) * nUn, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(g.ev[4], s));
    HIP_CHECK(hipEventSynchronize(g.ev[4]));
    float measure = 0, gather = 0, down = 0;
    HIP_CHECK(hipEventElapsedTime(&measure, g.ev[0], g.ev[1]));
    HIP_CHECK(hipEventElapsedTime(&gather, g.ev[2], g.ev[3]));
    HIP_CHECK(hipEventElapsedTime(&down, g.ev[3], g.ev[4]));
    box->pub.kernel_ms = (double)measure + gather; box->pub.d2h_ms = down;
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // (nothing of this call is still in flight when its buffers go)
    freeSummaryBox(box);
    throw;
  }
}

}  // namespace

extern "C" {

void xm_summary_free(xm_batch_summary* summary) {
  if (summary) freeSummaryBox((SummaryBox*)summary);  // pub is the first member
}

int xm_summary_last(xm_index* idx, int32_t want_unaligned, xm_batch_summary** out) {
  return lastCallEntry(idx, out, "xm_summary_last", [&] {
    const ResultStage::LastStreams last = lastCall(idx, "xm_summary_last");
    return &summaryRun(idx->summary, last.streams(idx->host().numContigs()), last.nq, want_unaligned != 0, idx->stream)->pub;
  });
}

}  // extern "C"
