// xm_sam_set_contigs, xm_sam_format_last (included once, by xm_capi.hip): the SAM records of the last align call formatted by the kernels of xm_sam.h from the
// streams and the batch where they lie in HBM - xm_pileup_add_last's contract (the context's mutex and stream, ResultStage::lastStreams) - and copied to a
// pinned buffer of the library's pool, so that the host's share of the SAM output is one write per batch.  samFormat is the part that xm_test_sam_format
// (xm_capi_test.h) runs over host-given arrays as well.
#pragma once

namespace {

// xm_sam_text plus what xm_sam_text_free needs to know about its buffer
struct SamBox {
  xm_sam_text pub;
  size_t bytesText;
};

void freeSamBox(SamBox* box) {
  g_pinned->put(box->pub.text, box->bytesText);
  free(box);
}

// the contig names one behind the other and their offsets -> HBM
void samUploadContigs(SamStage& g, int32_t n, const char* const* names) {
  std::string all;
  std::vector<int64_t> off((size_t)n + 1, 0);
  for (int32_t i = 0; i < n; i++) {
    if (!names[i]) throw std::runtime_error("contig " + std::to_string(i) + " has no name");
    all += names[i];
    off[(size_t)i + 1] = (int64_t)all.size();
  }
  g.dContigNames.ensure(all.size()); g.dContigOff.ensure((size_t)n + 1);
  if (!all.empty()) HIP_CHECK(hipMemcpy(g.dContigNames.p, all.data(), all.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(g.dContigOff.p, off.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  g.numContigs = n;
}

// offsets of names as xmio_batch has them: 2 * nq + 1 entries from 0 on, never falling -> the bytes of the names
int64_t samCheckNameOffsets(const int64_t* off, int64_t nq) {
  if (off[0] != 0) throw std::runtime_error("name_off must start at 0");
  for (int64_t i = 0; i < 2 * nq; i++) if (off[i + 1] < off[i]) throw std::runtime_error("name_off falls at entry " + std::to_string(i + 1));
  return off[2 * nq];
}

// The three stages on stream s over a job whose batch, streams and contig names are in HBM (job.batch.names / nameOff: null when hostNames are given - they
// are copied up first, from memory that may be pageable).  Returns the text in a pinned buffer, or throws: a malformed slice gives no text.
SamBox* samFormat(SamStage& g, SamJob job, const xm_sam_names* hostNames, hipStream_t s) {
  const int64_t nq = job.batch.nq;
  g.ev.ready();
  int64_t nameBytes = 0;
  if (hostNames) {
    if (!hostNames->names || !hostNames->name_off) throw std::runtime_error("names and name_off must both be given");
    nameBytes = samCheckNameOffsets(hostNames->name_off, nq);
  }
  // everything that is sized by the queries (a buffer that grows frees the old one, which waits for the device: before anything is queued)
  g.dBytes.ensure((size_t)nq); g.dRecords.ensure((size_t)nq); g.dOffset.ensure((size_t)nq + 1); g.dBlockSums.ensure(xmScanSums(nq, 2)); g.dCtl.ensure(4);
  if (hostNames) {
    g.dNames.ensure((size_t)nameBytes); g.dNameOff.ensure((size_t)(2 * nq + 1));
    job.batch.names = g.dNames.p; job.batch.nameOff = g.dNameOff.p;
  }
  SamBox* box = (SamBox*)calloc(1, sizeof(SamBox));
  if (!box) throw std::runtime_error("out of host memory");
  try {
    unsigned long long ctl[4] = {XM_NO_QUERY, 0, 0, 0};
    HIP_CHECK(hipEventRecord(g.ev[0], s));
    HIP_CHECK(hipMemcpyAsync(g.dCtl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    if (hostNames) {
      if (nameBytes) HIP_CHECK(hipMemcpyAsync(g.dNames.p, hostNames->names, (size_t)nameBytes, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(g.dNameOff.p, hostNames->name_off, sizeof(int64_t) * (size_t)(2 * nq + 1), hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipEventRecord(g.ev[1], s));
    if (nq > 0) hipLaunchKernelGGL(xm_sam_measure_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, job, g.dBytes.p, g.dRecords.p, g.dCtl.p);
    xmScanTotals(SamSums{nq, g.dBytes.p, g.dRecords.p, g.dOffset.p, g.dCtl.p}, nq, g.dBlockSums, s);  // (a batch of 0 queries: the totals are still written)
    xmScanPlace(SamByteOffsets{nq, g.dBytes.p, g.dOffset.p}, nq, g.dBlockSums, s, SamSums::N);
    HIP_CHECK(hipEventRecord(g.ev[2], s));
    HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    throwIfMalformed(ctl[0]);
    const size_t total = (size_t)ctl[2];
    g.dText.ensure(total);
    box->pub.text = (char*)g_pinned->get(total ? total : 1, &box->bytesText);
    box->pub.bytes = (int64_t)total;
    box->pub.records = (int64_t)ctl[3];
    box->pub.store = box;
    HIP_CHECK(hipEventRecord(g.ev[3], s));
    if (total) {
      const unsigned waves = (unsigned)std::min<int64_t>(nq, 16384);  // (a wavefront takes every waves-th query)
      hipLaunchKernelGGL(xm_sam_write_kernel, dim3(waves), dim3(64), 0, s, job, (const long long*)g.dOffset.p, g.dText.p, g.dCtl.p);
      HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(g.ev[4], s));
    if (total) HIP_CHECK(hipMemcpyAsync(box->pub.text, g.dText.p, total, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ctl, g.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(g.ev[5], s));
    HIP_CHECK(hipEventSynchronize(g.ev[5]));
    if (ctl[1] != 0) throw std::runtime_error("internal error: the text of " + std::to_string(ctl[1]) + " queries did not end where it was measured to");
    float up = 0, measure = 0, write = 0, down = 0;
    HIP_CHECK(hipEventElapsedTime(&up, g.ev[0], g.ev[1]));
    HIP_CHECK(hipEventElapsedTime(&measure, g.ev[1], g.ev[2]));
    HIP_CHECK(hipEventElapsedTime(&write, g.ev[3], g.ev[4]));
    HIP_CHECK(hipEventElapsedTime(&down, g.ev[4], g.ev[5]));
    box->pub.h2d_ms = up; box->pub.kernel_ms = (double)measure + write; box->pub.d2h_ms = down;
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // (nothing of this call is still in flight when its buffers go)
    if (box->pub.text) freeSamBox(box); else free(box);
    throw;
  }
}

}  // namespace

extern "C" {

int32_t xm_sam_tile_bytes(void) { return XM_SAM_TILE_BYTES; }

void xm_sam_text_free(xm_sam_text* t) {
  if (t) freeSamBox((SamBox*)t);  // pub is the first member
}

int xm_sam_set_contigs(xm_index* idx, int32_t num_contigs, const char* const* names) {
  if (!idx || !names) return fail("xm_sam_set_contigs: null argument");
  if (idx->hostOnly) return fail("xm_sam_set_contigs: index was built with host_only=1");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    if (num_contigs != idx->host().numContigs())
      throw std::runtime_error(std::to_string(num_contigs) + " names for an index of " + std::to_string(idx->host().numContigs()) + " contigs");
    HIP_CHECK(hipSetDevice(idx->device));
    HIP_CHECK(hipStreamSynchronize(idx->stream));
    samUploadContigs(idx->sam, num_contigs, names);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_sam_set_contigs: ") + e.what()); }
}

int xm_sam_format_last(xm_index* idx, const xm_sam_names* names, xm_sam_text** out) {
  return lastCallEntry(idx, out, "xm_sam_format_last", [&] {
    if (idx->sam.numContigs < 0) throw std::runtime_error("the contig names are not set (call xm_sam_set_contigs first)");
    const ResultStage::LastStreams last = lastCall(idx, "xm_sam_format_last");
    const DeviceBatch& d = idx->resident;
    if (!names && !d.hasNames)
      throw std::runtime_error("the resident batch has no names in HBM (it was staged from arrays, not by xm_batch_stage_fastq): hand the names in");
    SamJob job;
    job.batch = xm::SamBatch{last.nq, d.mateCount.p, d.mateOffset.p, d.mateLength.p, d.codes.p, names ? nullptr : d.names.p, names ? nullptr : d.nameOff.p};
    job.streams = last.streams(idx->sam.numContigs);  // (xm_sam_set_contigs takes as many names as the index has contigs, no other number)
    job.contigs = xm::SamContigs{idx->sam.numContigs, idx->sam.dContigNames.p, idx->sam.dContigOff.p};
    return &samFormat(idx->sam, job, names, idx->stream)->pub;
  });
}

}  // extern "C"
