// xm_unaligned_format_last, xm_context_set_batch_copy (included once, by xm_capi.hip, behind xm_capi_sam.h and xm_capi_summary.h): the unaligned-query file's
// text of the last align call made by the kernels of xm_unaligned.h from the batch and the streams where they lie in HBM - xm_summary_last's contract (the
// context's mutex and stream, ResultStage::lastStreams) - and copied to a pinned buffer of the library's pool; and the switch that then lets a batch staged
// from text stay in HBM.  unalignedFormat is the part that xm_test_unaligned_format (xm_capi_test.h) runs over host-given arrays as well.
#pragma once

namespace {

// The four stages on stream s over a batch and streams in HBM.  Returns the text in a pinned buffer (an xm_sam_text: records = the mates written, h2d_ms = 0), or
// throws: a malformed slice gives no text.  Nothing is launched for a batch of 0 queries, and nothing behind the totals for one without an unaligned query.
SamBox* unalignedFormat(UnalignedStage& g, const xm::UnalignedBatch& b, const xm::ResultStreams& st, hipStream_t s) {
  const int64_t nq = b.nq;
  SamBox* box = (SamBox*)calloc(1, sizeof(SamBox));
  if (!box) throw std::runtime_error("out of host memory");
  box->pub.store = box;
  try {
    if (nq == 0) {  // (a text of 0 bytes still has a buffer to give back, as xm_sam_format_last's has)
      box->pub.text = (char*)g_pinned->get(1, &box->bytesText);
      return box;
    }
    g.ev.ready();
    // everything that is sized by the queries (a buffer that grows frees the old one, which waits for the device: before anything is queued)
    g.dBytes.ensure((size_t)nq); g.dFlag.ensure((size_t)nq); g.dOff.ensure((size_t)nq + 1); g.dUoff.ensure((size_t)nq + 1);
    g.dBlockSums.ensure(xmScanSums(nq, 2)); g.dCtl.ensure(XM_UNALIGNED_CTL_WORDS);
    const unsigned grid = (unsigned)((nq + 255) / 256);
    unsigned long long ctl[XM_UNALIGNED_CTL_WORDS] = {XM_NO_QUERY, 0, XM_NO_QUERY, 0};
    int64_t totals[2] = {0, 0};
    HIP_CHECK(hipEventRecord(g.ev[0], s));
    HIP_CHECK(hipMemcpyAsync(g.dCtl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(xm_unaligned_measure_kernel, dim3(grid), dim3(256), 0, s, b, st, g.dBytes.p, g.dFlag.p, g.dCtl.p);
    xmScan(XmOffsets<int32_t, 2>{nq, {g.dBytes.p, g.dFlag.p}, {g.dOff.p, g.dUoff.p}}, nq, g.dBlockSums, s);
    HIP_CHECK(hipEventRecord(g.ev[1], s));
    HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[0], g.dOff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[1], g.dUoff.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the one wait for the totals and the control words)
    throwIfMalformed(ctl[0]);
    if (ctl[2] != XM_NO_QUERY) throw std::runtime_error("the record of query " + std::to_string(ctl[2]) + " is longer than 2^31 - 1 bytes");
    const size_t total = (size_t)totals[0], nUn = (size_t)totals[1];
    float measure = 0, write = 0, down = 0;
    HIP_CHECK(hipEventElapsedTime(&measure, g.ev[0], g.ev[1]));
    box->pub.records = (int64_t)ctl[1];
    box->pub.text = (char*)g_pinned->get(total ? total : 1, &box->bytesText);
    box->pub.bytes = (int64_t)total;
    if (total && nUn) {
      g.dList.ensure(nUn); g.dText.ensure(total);
      HIP_CHECK(hipEventRecord(g.ev[2], s));
      hipLaunchKernelGGL(xm_unaligned_compact_kernel, dim3(grid), dim3(256), 0, s, (long long)nq, (const int64_t*)g.dUoff.p, g.dList.p, (long long)nUn);
      const unsigned waves = (unsigned)std::min<size_t>(nUn, 16384);  // (a wavefront takes every waves-th entry of the list)
      hipLaunchKernelGGL(xm_unaligned_write_kernel, dim3(waves), dim3(64), 0, s, b, (const int64_t*)g.dList.p, (long long)nUn, (const int64_t*)g.dOff.p, g.dText.p, (long long)total, g.dCtl.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(g.ev[3], s));
      HIP_CHECK(hipMemcpyAsync(box->pub.text, g.dText.p, total, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(g.ev[4], s));
      HIP_CHECK(hipEventSynchronize(g.ev[4]));
      if (ctl[3] != 0) throw std::runtime_error("internal error: the records of " + std::to_string(ctl[3]) + " queries did not end where they were measured to");
      HIP_CHECK(hipEventElapsedTime(&write, g.ev[2], g.ev[3]));
      HIP_CHECK(hipEventElapsedTime(&down, g.ev[3], g.ev[4]));
    }
    box->pub.kernel_ms = (double)measure + write; box->pub.d2h_ms = down;
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // (nothing of this call is still in flight when its buffers go)
    if (box->pub.text) freeSamBox(box); else free(box);
    throw;
  }
}

}  // namespace

extern "C" {

int xm_unaligned_format_last(xm_index* idx, xm_sam_text** out) {
  return lastCallEntry(idx, out, "xm_unaligned_format_last", [&] {
    const ResultStage::LastStreams last = lastCall(idx, "xm_unaligned_format_last");
    const DeviceBatch& d = idx->resident;
    if (!d.hasNames)
      throw std::runtime_error("the resident batch has no names in HBM (it was staged from arrays, not by xm_batch_stage_fastq or xm_batch_stage_fasta)");
    const bool q = d.hasQuals;
    const xm::UnalignedBatch b{last.nq, d.mateCount.p, d.mateOffset.p, d.mateLength.p, d.codes.p, d.codesLength, d.names.p, d.nameOff.p, d.namesLength,
                               q ? d.quals.p : nullptr, q ? d.qualOff.p : nullptr, q ? d.hasQual.p : nullptr, q ? d.qualsLength : 0};
    return &unalignedFormat(idx->unaligned, b, last.streams(idx->host().numContigs()), idx->stream)->pub;
  });
}

int xm_context_set_batch_copy(xm_index* idx, int32_t on) {
  if (!idx) return fail("xm_context_set_batch_copy: null argument");
  std::lock_guard<std::mutex> stageLock(idx->stageMu);  // (the staging calls read it under this lock)
  idx->batchCopy = on != 0;
  return 0;
}

}  // extern "C"
