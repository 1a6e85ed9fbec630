// xm_batch_stage_fastq (included once, by xm_capi.hip): the staged batch built from FASTQ text by the kernels of xm_fastq.h.  What xm_batch_stage does -
// stageMu, the context's `staged` DeviceBatch, the GPU's staging stream - with the text copied up instead of the arrays, and the arrays, names and
// qualities copied down into pinned buffers for the host's writers.  The host does no work per record but the facts it needs of the returned
// mate lengths (validateBatch: longest mate, any pair, the lengths the confidence table is seeded for).
#pragma once

namespace {

// xm_fastq_batch plus what xm_fastq_batch_free needs to know about its buffers
struct FastqBox {
  xm_fastq_batch pub;
  size_t bytes[9];
};

void freeFastqBox(FastqBox* box) {
  xm_fastq_batch& b = box->pub;
  void* const bufs[9] = {b.mate_count, b.mate_offset, b.mate_length, b.codes, b.names, b.name_off, b.quals, b.qual_off, b.has_qual};
  for (int i = 0; i < 9; i++) g_pinned->put(bufs[i], box->bytes[i]);
  free(box);
}

std::string fastqWhere(int file, long long record) { return "file " + std::to_string(file + 1) + " record " + std::to_string(record) + ": "; }

// the text up and stage 1 of xm_fastq.h (the line ends) on stream s
void fastqLines(FastqStage& f, const xm_fastq_text* t, const FastqText texts[2], bool paired, hipStream_t s) {
  FastqCtl ctl0;
  memset(&ctl0, 0, sizeof(ctl0));
  ctl0.firstError = XM_FASTQ_NO_ERROR;
  HIP_CHECK(hipEventRecord(f.ev[0], s));
  HIP_CHECK(hipMemcpyAsync(f.dCtl.p, &ctl0, sizeof(ctl0), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(f.dText[0].p, t->text1, (size_t)t->bytes1, hipMemcpyHostToDevice, s));
  if (paired) HIP_CHECK(hipMemcpyAsync(f.dText[1].p, t->text2, (size_t)t->bytes2, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipEventRecord(f.ev[1], s));
  for (int k = 0; k < (paired ? 2 : 1); k++) {
    const long long nTiles = (texts[k].bytes + XM_FASTQ_TILE_BYTES - 1) / XM_FASTQ_TILE_BYTES;
    hipLaunchKernelGGL(xm_fastq_count_kernel, dim3((unsigned)nTiles), dim3(256), 0, s, texts[k]);
    hipLaunchKernelGGL(xm_fastq_tiles_kernel, dim3(1), dim3(256), 0, s, texts[k], nTiles, k, f.dCtl.p);
    hipLaunchKernelGGL(xm_fastq_ends_kernel, dim3((unsigned)nTiles), dim3(256), 0, s, texts[k]);
  }
}

// stage 3 (the offsets of the mate slots, the totals) on stream s (queued; the caller waits for ev[2])
void fastqOffsets(FastqStage& f, DeviceBatch& d, long long slots, bool keepQual, hipStream_t s) {
  xmScan(FastqMateOffsets{slots, f.dMates.p, keepQual ? 1 : 0, d.mateOffset.p, d.nameOff.p, keepQual ? d.qualOff.p : nullptr, f.dCtl.p}, slots, f.dBlockSums, s);
  HIP_CHECK(hipEventRecord(f.ev[2], s));
}

// the stages of xm_fastq.h on stream s, up to the totals (queued; the caller waits for ev[2])
void fastqParse(FastqStage& f, DeviceBatch& d, const xm_fastq_text* t, const FastqText texts[2], int64_t nq, bool paired, bool keepQual, hipStream_t s) {
  const long long slots = 2 * nq;
  fastqLines(f, t, texts, paired, s);
  FastqFieldsOut out{f.dMates.p, d.mateCount.p, d.mateLength.p, d.expected.p, d.deviation.p, d.hasQual.p, f.dCtl.p};
  hipLaunchKernelGGL(xm_fastq_fields_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, texts[0], texts[1], (long long)nq, paired ? 1 : 0, t->expected_inner, t->deviation, out);
  fastqOffsets(f, d, slots, keepQual, s);
}

// the split form's stage 2b (the records' first queries) behind whatever made the section counts, on stream s; the caller reads FastqCtl::sections behind ev[6]
void fastqSplitFirst(FastqStage& f, long long records, hipStream_t s) {
  xmScan(FastqSplitFirst{records, f.dRecCount.p, f.dRecFirst.p, f.dCtl.p}, records, f.dRecBlockSums, s);
  HIP_CHECK(hipEventRecord(f.ev[6], s));
}

// the split form: the text up, stage 1, stages 2a and 2b on stream s
void fastqSplitRecords(FastqStage& f, const xm_fastq_text* t, const FastqText texts[2], hipStream_t s) {
  const long long records = texts[0].records;
  fastqLines(f, t, texts, false, s);
  hipLaunchKernelGGL(xm_fastq_split_records_kernel, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, s, texts[0], (long long)t->split_past_size, f.dRecs.p, f.dRecCount.p, f.dCtl.p);
  fastqSplitFirst(f, records, s);
}

// the split form: stage 2c (a lane per section) and stage 3 over the section slots, which the caller has sized for nq queries
void fastqSplitSections(FastqStage& f, DeviceBatch& d, long long records, int64_t nq, bool keepQual, hipStream_t s) {
  HIP_CHECK(hipEventRecord(f.ev[7], s));
  FastqFieldsOut out{f.dMates.p, d.mateCount.p, d.mateLength.p, d.expected.p, d.deviation.p, d.hasQual.p, f.dCtl.p};
  hipLaunchKernelGGL(xm_fastq_split_sections_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (long long)nq, records, (const FastqMate*)f.dRecs.p, (const int64_t*)f.dRecFirst.p, out);
  fastqOffsets(f, d, 2 * nq, keepQual, s);
}

// what the host reads of FastqCtl behind stage 2: a record that is not of the strict form comes first (an empty line between two records also makes the line count wrong)
void fastqCheckText(const FastqCtl& ctl, const FastqText texts[2], bool paired) {
  if (ctl.firstError != XM_FASTQ_NO_ERROR)
    throw std::runtime_error(fastqWhere((int)(ctl.firstError >> 48), (long long)((ctl.firstError >> 8) & 0xFFFFFFFFFFull)) + fastqErrorText((int)(ctl.firstError & 0xFF)));
  for (int k = 0; k < (paired ? 2 : 1); k++)
    if (ctl.lines[k] != 4 * texts[k].records)
      throw std::runtime_error(fastqWhere(k, std::min(ctl.lines[k] / 4, texts[k].records)) + fastqErrorText(XM_FQ_LINE_COUNT) + " (" + std::to_string(ctl.lines[k]) + " lines, " +
                               std::to_string(texts[k].records) + " records announced)");
}

// What the entries that stage a batch from text do behind stage 3 (xm_batch_stage_fastq, and xm_batch_stage_fasta of xm_capi_fasta.h): the arrays the totals size, stage 4
// (launchGather queues it on the stream it is given), everything down into the box's pinned buffers (copyBatch off: the mate counts, offsets and lengths only), the times of the call's parts, and the host's facts of the batch.
// splitWaits: the call waited for the section count between ev[6] and ev[7].
template <class LaunchGather>
void fastqFinish(xm_index* idx, FastqBox* box, const FastqCtl& ctl, int64_t nq, bool keepQual, bool copyBatch, bool splitWaits, LaunchGather&& launchGather) {
  DeviceBatch& d = idx->staged;
  FastqStage& f = idx->fastq;
  xm_fastq_batch& b = box->pub;
  const long long slots = 2 * nq;
  // the arrays the totals size, stage 4, everything down
  const size_t nCodes = (size_t)ctl.totals[0], nNames = (size_t)ctl.totals[1], nQuals = (size_t)ctl.totals[2];
  d.codes.ensure(nCodes);
  d.names.ensure(nNames);
  if (keepQual) d.quals.ensure(nQuals);
  b.codes_length = (int64_t)nCodes;
  if (copyBatch) {
    b.codes = (uint8_t*)g_pinned->get(nCodes, &box->bytes[3]);
    b.names = (char*)g_pinned->get(nNames, &box->bytes[4]);
    if (keepQual) b.quals = (char*)g_pinned->get(nQuals, &box->bytes[6]);
  }
  idx->dt->onStagingStream([&](hipStream_t s) {
    HIP_CHECK(hipEventRecord(f.ev[3], s));
    launchGather(s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(f.ev[4], s));
    HIP_CHECK(hipMemcpyAsync(b.mate_count, d.mateCount.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(b.mate_offset, d.mateOffset.p, sizeof(int64_t) * (size_t)slots, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(b.mate_length, d.mateLength.p, sizeof(int32_t) * (size_t)slots, hipMemcpyDeviceToHost, s));
    if (copyBatch) {
      HIP_CHECK(hipMemcpyAsync(b.name_off, d.nameOff.p, sizeof(int64_t) * (size_t)(slots + 1), hipMemcpyDeviceToHost, s));
      if (nCodes) HIP_CHECK(hipMemcpyAsync(b.codes, d.codes.p, nCodes, hipMemcpyDeviceToHost, s));
      if (nNames) HIP_CHECK(hipMemcpyAsync(b.names, d.names.p, nNames, hipMemcpyDeviceToHost, s));
    }
    if (keepQual && copyBatch) {
      HIP_CHECK(hipMemcpyAsync(b.qual_off, d.qualOff.p, sizeof(int64_t) * (size_t)(slots + 1), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(b.has_qual, d.hasQual.p, (size_t)slots, hipMemcpyDeviceToHost, s));
      if (nQuals) HIP_CHECK(hipMemcpyAsync(b.quals, d.quals.p, nQuals, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipEventRecord(f.ev[5], s));
  });
  HIP_CHECK(hipEventSynchronize(f.ev[5]));
  float up = 0, parse = 0, gather = 0, down = 0;
  HIP_CHECK(hipEventElapsedTime(&up, f.ev[0], f.ev[1]));
  if (splitWaits) {  // (not the time the host took between the two to size the slots)
    float records = 0;
    HIP_CHECK(hipEventElapsedTime(&records, f.ev[1], f.ev[6]));
    HIP_CHECK(hipEventElapsedTime(&parse, f.ev[7], f.ev[2]));
    parse += records;
  } else HIP_CHECK(hipEventElapsedTime(&parse, f.ev[1], f.ev[2]));
  HIP_CHECK(hipEventElapsedTime(&gather, f.ev[3], f.ev[4]));
  HIP_CHECK(hipEventElapsedTime(&down, f.ev[4], f.ev[5]));
  b.h2d_ms = up; b.kernel_ms = (double)parse + gather; b.d2h_ms = down;
  // the host's facts of the batch, from the returned mate lengths
  xm_query_batch view;
  memset(&view, 0, sizeof(view));
  view.num_queries = nq; view.mate_count = b.mate_count; view.mate_offset = b.mate_offset; view.mate_length = b.mate_length; view.codes = b.codes; view.codes_length = b.codes_length;
  bool anyPaired = false;
  const int maxLen = validateBatch(&view, &anyPaired, &d.lens);
  d.anyPaired = anyPaired;
  idx->ensureTablesFor(maxLen);  // (tables that grow wait for the launches that read them: DeviceTables::rw)
  d.maxLen = maxLen;
  d.h2dMs = up;
  d.hasNames = true;
  d.hasQuals = keepQual;
  d.codesLength = (int64_t)nCodes; d.namesLength = (int64_t)nNames; d.qualsLength = keepQual ? (int64_t)nQuals : 0;
  d.nq = nq;
}

}  // namespace

extern "C" {

int32_t xm_fastq_tile_bytes(void) { return XM_FASTQ_TILE_BYTES; }

void xm_fastq_batch_free(xm_fastq_batch* b) {
  if (b) freeFastqBox((FastqBox*)b);  // pub is the first member
}

int xm_batch_stage_fastq(xm_index* idx, const xm_fastq_text* t, xm_fastq_batch** outBatch) {
  if (!idx || !t || !outBatch) return fail("xm_batch_stage_fastq: null argument");
  *outBatch = nullptr;
  if (idx->hostOnly) return fail("xm_batch_stage_fastq: index was built with host_only=1");
  const bool paired = t->text2 != nullptr;
  const bool keepQual = t->keep_qualities != 0;
  const long long maxBytes = 1ll << 30;
  if (!t->text1 || t->records1 < 1 || t->bytes1 < 1 || t->bytes1 > maxBytes) return fail("xm_batch_stage_fastq: file 1 record 0: a text holds 1 .. 2^30 bytes and at least one record");
  if (paired && (t->records2 < 1 || t->bytes2 < 1 || t->bytes2 > maxBytes)) return fail("xm_batch_stage_fastq: file 2 record 0: a text holds 1 .. 2^30 bytes and at least one record");
  if (paired && t->records1 != t->records2) {
    const long long fewer = std::min(t->records1, t->records2);
    return fail("xm_batch_stage_fastq: " + fastqWhere(t->records1 < t->records2 ? 0 : 1, fewer) + "paired texts have different numbers of records (" + std::to_string(t->records1) + ", " +
                std::to_string(t->records2) + ")");
  }
  if (t->records1 > (1ll << 28)) return fail("xm_batch_stage_fastq: file 1 record 0: too many records for one text");
  const int split = t->split_past_size;
  if (split < 0) return fail("xm_batch_stage_fastq: file 1 record 0: split_past_size must be >= 0");
  if (split > 0 && paired) return fail("xm_batch_stage_fastq: file 2 record 0: pairs are not cut into sections (split_past_size is for single reads, as --split-queries-past-size is)");
  if (split > XM_FASTQ_MAX_MATE) return fail("xm_batch_stage_fastq: file 1 record 0: split_past_size out of range (0..30000: a section is a mate)");
  FastqBox* box = nullptr;
  try {
    std::lock_guard<std::mutex> stageLock(idx->stageMu);
    DeviceBatch& d = idx->staged;
    FastqStage& f = idx->fastq;
    d.nq = -1;
    d.h2dMs = 0;
    d.hasNames = false;
    d.hasQuals = false;
    HIP_CHECK(hipSetDevice(idx->device));
    f.ev.ready();
    box = (FastqBox*)calloc(1, sizeof(FastqBox));
    if (!box) throw std::runtime_error("out of host memory");
    xm_fastq_batch& b = box->pub;
    // everything that is sized by the records and the bytes (a buffer that grows frees the old one, which waits for the device: before the stream is taken)
    FastqText texts[2];
    memset(texts, 0, sizeof(texts));
    for (int k = 0; k < (paired ? 2 : 1); k++) {
      const long long bytes = k ? t->bytes2 : t->bytes1, records = k ? t->records2 : t->records1;
      f.dText[k].ensure((size_t)((bytes + 15) & ~15ll));
      f.dLineEnd[k].ensure((size_t)(4 * records + 1));
      f.dTileCount[k].ensure((size_t)((bytes + XM_FASTQ_TILE_BYTES - 1) / XM_FASTQ_TILE_BYTES));
      texts[k] = FastqText{f.dText[k].p, bytes, records, f.dLineEnd[k].p, f.dTileCount[k].p, 4 * records + 1};
    }
    f.dCtl.ensure(1);
    FastqCtl ctl;
    int64_t nq = t->records1;
    if (split > 0) {
      // the split form: the records' fields and the scan of their section counts first - the query count sizes everything per slot, so the host waits for it
      // (one wait more than without a split: three in the call)
      const long long records = t->records1;
      f.dRecs.ensure((size_t)records); f.dRecCount.ensure((size_t)records); f.dRecFirst.ensure((size_t)records + 1);
      f.dRecBlockSums.ensure(xmScanSums(records, 1));
      idx->dt->onStagingStream([&](hipStream_t s) {
        fastqSplitRecords(f, t, texts, s);
        HIP_CHECK(hipMemcpyAsync(&ctl, f.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
      });
      fastqCheckText(ctl, texts, false);
      nq = ctl.sections;
      if (nq < records || nq > t->bytes1) throw std::runtime_error("internal: " + std::to_string(nq) + " sections of " + std::to_string(records) + " records");
      if (nq > (1ll << 28)) throw std::runtime_error(fastqWhere(0, 0) + "too many sections for one text (" + std::to_string(nq) + ")");
    }
    const long long slots = 2 * nq;
    f.dMates.ensure((size_t)slots); d.hasQual.ensure((size_t)slots);
    f.dBlockSums.ensure(xmScanSums(slots, 3));
    d.nameOff.ensure((size_t)slots + 1);
    if (keepQual) d.qualOff.ensure((size_t)slots + 1);
    d.mateCount.ensure((size_t)nq); d.mateOffset.ensure((size_t)slots); d.mateLength.ensure((size_t)slots);
    d.expected.ensure((size_t)nq); d.deviation.ensure((size_t)nq);
    b.num_queries = nq;
    b.mate_count = (int32_t*)g_pinned->get(sizeof(int32_t) * (size_t)nq, &box->bytes[0]);
    b.mate_offset = (int64_t*)g_pinned->get(sizeof(int64_t) * (size_t)slots, &box->bytes[1]);
    b.mate_length = (int32_t*)g_pinned->get(sizeof(int32_t) * (size_t)slots, &box->bytes[2]);
    const bool copyBatch = idx->batchCopy;  // (xm_context_set_batch_copy(0): the six arrays below and in fastqFinish stay in HBM, and no pinned buffer is taken for them)
    if (copyBatch) b.name_off = (int64_t*)g_pinned->get(sizeof(int64_t) * (size_t)(slots + 1), &box->bytes[5]);
    if (keepQual && copyBatch) {
      b.qual_off = (int64_t*)g_pinned->get(sizeof(int64_t) * (size_t)(slots + 1), &box->bytes[7]);
      b.has_qual = (uint8_t*)g_pinned->get((size_t)slots, &box->bytes[8]);
    }
    // text up, stages 1 to 3 (with a split: stages 2c and 3), the control words down
    idx->dt->onStagingStream([&](hipStream_t s) {
      if (split > 0) fastqSplitSections(f, d, t->records1, nq, keepQual, s);
      else fastqParse(f, d, t, texts, nq, paired, keepQual, s);
      HIP_CHECK(hipMemcpyAsync(&ctl, f.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));  // (under the stream's lock: the copy lands in this frame)
    });
    if (split == 0) fastqCheckText(ctl, texts, paired);
    else if (ctl.sections != nq) throw std::runtime_error("internal: the section count changed between two launches");
    fastqFinish(idx, box, ctl, nq, keepQual, copyBatch, split > 0, [&](hipStream_t s) {
      hipLaunchKernelGGL(xm_fastq_gather_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, s, slots, (const FastqMate*)f.dMates.p, (const char*)f.dText[0].p, (const char*)f.dText[1].p,
                         (const int64_t*)d.mateOffset.p, (const int64_t*)d.nameOff.p, (const int64_t*)(keepQual ? d.qualOff.p : nullptr), d.codes.p, d.names.p,
                         keepQual ? d.quals.p : nullptr);
    });
    *outBatch = &box->pub;
    return 0;
  } catch (std::exception& e) {
    if (box) freeFastqBox(box);
    return fail(std::string("xm_batch_stage_fastq: ") + e.what());
  }
}

}  // extern "C"
