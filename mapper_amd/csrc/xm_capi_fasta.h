// xm_batch_stage_fasta (included once, by xm_capi.hip, behind xm_capi_fastq.h): the staged batch built from FASTA text by the kernels of xm_fasta.h.  The
// contract, the buffers and the returned xm_fastq_batch are xm_batch_stage_fastq's (stageMu, the context's `staged` DeviceBatch, the GPU's staging stream,
// FastqStage, fastqOffsets, fastqFinish); what differs is what lies between the line ends and the mate slots, and the gather.
#pragma once

namespace {

// stages 1 to 3 of xm_fasta.h on stream s: the text up, the line ends, the lines, the two scans over them
void fastaLines(FastqStage& f, const xm_fastq_text* up, const FastqText texts[2], const FastaLines lines[2], bool paired, hipStream_t s) {
  fastqLines(f, up, texts, paired, s);
  for (int k = 0; k < (paired ? 2 : 1); k++) {
    const long long n = lines[k].lines;
    hipLaunchKernelGGL(xm_fasta_lines_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, texts[k], lines[k], k, f.dCtl.p);
    xmScan(FastaLineOffsets{lines[k], texts[k].records, k, f.dCtl.p}, n, f.dLineBlockSums[k], s);  // (n announced: the grid; the kernels stop at the lines kept)
  }
}

// what the host reads of FastqCtl: a refusal with its record comes first, then a text that does not hold what was announced
void fastaCheckText(const FastqCtl& ctl, const FastqText texts[2], const FastaLines lines[2], bool paired) {
  if (ctl.firstError != XM_FASTQ_NO_ERROR)
    throw std::runtime_error(fastqWhere((int)((ctl.firstError >> 48) & 1), (long long)((ctl.firstError >> 8) & 0xFFFFFFFFFFull)) + fastaErrorText((int)(ctl.firstError & 0xFF)));
  for (int k = 0; k < (paired ? 2 : 1); k++) {
    const long long record = std::min(ctl.headers[k], texts[k].records);
    if (ctl.lines[k] != lines[k].lines)
      throw std::runtime_error(fastqWhere(k, record) + fastaErrorText(XM_FA_LINE_COUNT) + " (" + std::to_string(ctl.lines[k]) + " lines, " + std::to_string(lines[k].lines) + " announced)");
    if (ctl.headers[k] != texts[k].records)
      throw std::runtime_error(fastqWhere(k, record) + fastaErrorText(XM_FA_RECORD_COUNT) + " (" + std::to_string(ctl.headers[k]) + " headers, " + std::to_string(texts[k].records) +
                               " records announced)");
  }
}

}  // namespace

extern "C" {

int xm_batch_stage_fasta(xm_index* idx, const xm_fasta_text* t, xm_fastq_batch** outBatch) {
  if (!idx || !t || !outBatch) return fail("xm_batch_stage_fasta: null argument");
  *outBatch = nullptr;
  if (idx->hostOnly) return fail("xm_batch_stage_fasta: index was built with host_only=1");
  const bool paired = t->text2 != nullptr;
  const bool keepQual = t->keep_qualities != 0;
  const long long maxBytes = 1ll << 30;
  if (!t->text1 || t->records1 < 1 || t->bytes1 < 1 || t->bytes1 > maxBytes) return fail("xm_batch_stage_fasta: file 1 record 0: a text holds 1 .. 2^30 bytes and at least one record");
  if (paired && (t->records2 < 1 || t->bytes2 < 1 || t->bytes2 > maxBytes)) return fail("xm_batch_stage_fasta: file 2 record 0: a text holds 1 .. 2^30 bytes and at least one record");
  if (paired && t->records1 != t->records2) {
    const long long fewer = std::min(t->records1, t->records2);
    return fail("xm_batch_stage_fasta: " + fastqWhere(t->records1 < t->records2 ? 0 : 1, fewer) + "paired texts have different numbers of records (" + std::to_string(t->records1) + ", " +
                std::to_string(t->records2) + ")");
  }
  for (int k = 0; k < (paired ? 2 : 1); k++) {
    const long long lines = k ? t->lines2 : t->lines1, records = k ? t->records2 : t->records1, bytes = k ? t->bytes2 : t->bytes1;
    if (lines < records || lines > XM_FASTA_MAX_LINES || lines > bytes + 1)
      return fail("xm_batch_stage_fasta: " + fastqWhere(k, 0) + "a text holds at least a line a record, at most 2^26 lines, and no more lines than bytes + 1 (" + std::to_string(lines) +
                  " lines announced)");
  }
  const int split = t->split_past_size;
  if (split < 0) return fail("xm_batch_stage_fasta: file 1 record 0: split_past_size must be >= 0");
  if (split > 0 && paired) return fail("xm_batch_stage_fasta: file 2 record 0: pairs are not cut into sections (split_past_size is for single reads, as --split-queries-past-size is)");
  if (split > XM_FASTQ_MAX_MATE) return fail("xm_batch_stage_fasta: file 1 record 0: split_past_size out of range (0..30000: a section is a mate)");
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
    // everything that is sized by the bytes, the lines and the records (a buffer that grows frees the old one, which waits for the device: before the stream is taken)
    FastqText texts[2];
    FastaLines lines[2];
    FastaGatherText gather[2];
    memset(texts, 0, sizeof(texts));
    memset(lines, 0, sizeof(lines));
    memset(gather, 0, sizeof(gather));
    for (int k = 0; k < (paired ? 2 : 1); k++) {
      const long long bytes = k ? t->bytes2 : t->bytes1, records = k ? t->records2 : t->records1, n = k ? t->lines2 : t->lines1;
      f.dText[k].ensure((size_t)((bytes + 15) & ~15ll));
      f.dLineEnd[k].ensure((size_t)n + 1);
      f.dTileCount[k].ensure((size_t)((bytes + XM_FASTQ_TILE_BYTES - 1) / XM_FASTQ_TILE_BYTES));
      f.dLineStart[k].ensure((size_t)n); f.dLineBases[k].ensure((size_t)n); f.dLineHeader[k].ensure((size_t)n);
      f.dBaseBefore[k].ensure((size_t)n + 1); f.dRecLine[k].ensure((size_t)records + 1);
      f.dLineBlockSums[k].ensure(xmScanSums(n, 2));
      texts[k] = FastqText{f.dText[k].p, bytes, records, f.dLineEnd[k].p, f.dTileCount[k].p, n + 1};
      lines[k] = FastaLines{n, f.dLineStart[k].p, f.dLineBases[k].p, f.dLineHeader[k].p, f.dBaseBefore[k].p, f.dRecLine[k].p};
      gather[k] = FastaGatherText{f.dText[k].p, bytes, f.dLineStart[k].p, f.dBaseBefore[k].p, n};
    }
    f.dCtl.ensure(1);
    // (fastqLines copies the texts up by xm_fastq_text's fields: the two structs name them alike up to the lines)
    xm_fastq_text up;
    memset(&up, 0, sizeof(up));
    up.text1 = t->text1; up.bytes1 = t->bytes1; up.records1 = t->records1;
    up.text2 = t->text2; up.bytes2 = t->bytes2; up.records2 = t->records2;
    FastqCtl ctl;
    int64_t nq = t->records1;
    if (split > 0) {
      // the split form: the records' ordinals and the scan of their section counts first - the query count sizes everything per slot, so the host waits for
      // it, exactly as xm_batch_stage_fastq does (three waits in the call)
      const long long records = t->records1;
      f.dRecs.ensure((size_t)records); f.dRecCount.ensure((size_t)records); f.dRecFirst.ensure((size_t)records + 1);
      f.dRecBlockSums.ensure(xmScanSums(records, 1));
      idx->dt->onStagingStream([&](hipStream_t s) {
        fastaLines(f, &up, texts, lines, false, s);
        hipLaunchKernelGGL(xm_fasta_split_records_kernel, dim3((unsigned)((records + 255) / 256)), dim3(256), 0, s, texts[0], lines[0], (long long)split, f.dRecs.p, f.dRecCount.p, f.dCtl.p);
        fastqSplitFirst(f, records, s);
        HIP_CHECK(hipMemcpyAsync(&ctl, f.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
      });
      fastaCheckText(ctl, texts, lines, false);
      nq = ctl.sections;
      if (nq < records || nq > t->bytes1) throw std::runtime_error("internal: " + std::to_string(nq) + " sections of " + std::to_string(records) + " records");
      if (nq > (1ll << 28)) throw std::runtime_error(fastqWhere(0, 0) + "too many sections for one text (" + std::to_string(nq) + ")");
    }
    if (nq > (1ll << 28)) throw std::runtime_error(fastqWhere(0, 0) + "too many records for one text");
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
    // text up and stages 1 to 5 (with a split: the sections and stage 5), the control words down
    idx->dt->onStagingStream([&](hipStream_t s) {
      if (split > 0) fastqSplitSections(f, d, t->records1, nq, keepQual, s);
      else {
        fastaLines(f, &up, texts, lines, paired, s);
        FastqFieldsOut out{f.dMates.p, d.mateCount.p, d.mateLength.p, d.expected.p, d.deviation.p, d.hasQual.p, f.dCtl.p};
        hipLaunchKernelGGL(xm_fasta_records_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, texts[0], texts[1], lines[0], lines[1], (long long)nq, paired ? 1 : 0,
                           t->expected_inner, t->deviation, out);
        fastqOffsets(f, d, slots, keepQual, s);
      }
      HIP_CHECK(hipMemcpyAsync(&ctl, f.dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));  // (under the stream's lock: the copy lands in this frame)
    });
    if (split == 0) fastaCheckText(ctl, texts, lines, paired);
    else if (ctl.sections != nq) throw std::runtime_error("internal: the section count changed between two launches");
    fastqFinish(idx, box, ctl, nq, keepQual, copyBatch, split > 0, [&](hipStream_t s) {
      hipLaunchKernelGGL(xm_fasta_gather_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, s, slots, (const FastqMate*)f.dMates.p, gather[0], gather[1], (const int64_t*)d.mateOffset.p,
                         (const int64_t*)d.nameOff.p, d.codes.p, d.names.p);
    });
    *outBatch = &box->pub;
    return 0;
  } catch (std::exception& e) {
    if (box) freeFastqBox(box);
    return fail(std::string("xm_batch_stage_fasta: ") + e.what());
  }
}

}  // extern "C"
