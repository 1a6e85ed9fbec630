// The test-only entries of libxmapper_hip.so (included once, by xm_capi.hip): components of the align kernel run alone on given inputs.  Buffers and the
// error contract are here; the kernels stand behind the align kernel in xm_align_kernel.hip (TestLocalLaunch, TestBoundLaunch: xm_kernel_common.h).
#pragma once

namespace {

// Host-given result streams copied to HBM, to be walked like ResultStage::lastStreams' (the entries below check the offsets first)
struct TestStreams {
  DevBuf<int32_t> dInts;
  DevBuf<double> dDbls;
  DevBuf<int64_t> dIntOff, dDblOff;
  TestStreams(int64_t nq, const int32_t* ints, const double* dbls, const int64_t* intOff, const int64_t* dblOff) {
    const size_t nInts = (size_t)intOff[nq], nDbls = (size_t)dblOff[nq];
    dInts.ensure(nInts); dDbls.ensure(nDbls); dIntOff.ensure((size_t)nq + 1); dDblOff.ensure((size_t)nq + 1);
    if (nInts) HIP_CHECK(hipMemcpy(dInts.p, ints, sizeof(int32_t) * nInts, hipMemcpyHostToDevice));
    if (nDbls) HIP_CHECK(hipMemcpy(dDbls.p, dbls, sizeof(double) * nDbls, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIntOff.p, intOff, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dDblOff.p, dblOff, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyHostToDevice));
  }
  xm::ResultStreams streams(int32_t numContigs) const { return xm::ResultStreams{dInts.p, dDbls.p, dIntOff.p, dDblOff.p, numContigs}; }
};
const xm::ResultStreams kNoStreams{nullptr, nullptr, nullptr, nullptr, 0};  // of a batch of 0 queries: nothing is read

}  // namespace

extern "C" {

// Test-only, not declared in the header (tests/test_launch_const_layout.py binds it by name): the layout of the launch block as the host side, which writes
// it, was compiled (launchConstLayout, xm_defs.h).  out: XM_LAUNCH_CONST_LAYOUT_WORDS words.  Needs no GPU.
int xm_test_launch_const_layout(int64_t* out, int32_t cap) {
  if (!out || cap < XM_LAUNCH_CONST_LAYOUT_WORDS) return -1;
  launchConstLayout(out);
  return XM_LAUNCH_CONST_LAYOUT_WORDS;
}
// Test-only: what the rejection filter did in this thread's last xm_test_local_align call (searches taken, searches rejected, cells computed).
static thread_local int64_t g_testBound[3] = {0, 0, 0};
void xm_test_bound_counters(int64_t* out3) { for (int i = 0; i < 3; i++) out3[i] = g_testBound[i]; }

// Test-only entry (tests/test_gpu_bound.py): the rejection filter alone on one problem (xm_test_bound_kernel).  out3: taken, rejected, cells computed.
int xm_test_bound(int32_t device, const xm_params* p, const uint8_t* query, int32_t query_length, int32_t query_rc, int32_t start_a, int32_t end_a, const uint8_t* reference, int32_t reference_length,
                  int32_t start_b, int32_t end_b, int32_t predicted_best_offset, int32_t pair, int64_t* out3) {
  if (!p || !query || !reference || !out3) return fail("xm_test_bound: null argument");
  if (query_length < 1 || reference_length < 1 || start_a < 0 || end_a > query_length || start_a > end_a || start_b < 0 || end_b > reference_length || start_b > end_b) return fail("xm_test_bound: bad sections");
  try {
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    const Params params = paramsFromC(*p);
    DevBuf<uint8_t> dq, dr, dArena;
    DevBuf<int64_t> dOut;
    dq.ensure((size_t)query_length); dr.ensure((size_t)reference_length); dOut.ensure(4); dArena.ensure(64 * 1024);
    HIP_CHECK(hipMemcpy(dq.p, query, (size_t)query_length, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dr.p, reference, (size_t)reference_length, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dOut.p, 0, sizeof(int64_t) * 4));
    TestBoundLaunch t{};
    t.params = params; t.query = dq.p; t.queryLength = query_length; t.queryRc = query_rc; t.startA = start_a; t.endA = end_a;
    t.reference = dr.p; t.referenceLength = reference_length; t.startB = start_b; t.endB = end_b; t.predictedBestOffset = predicted_best_offset;
    t.pair = pair == 3 ? 3 : (pair ? 1 : 0); t.arena = dArena.p; t.arenaBytes = 64 * 1024; t.out = dOut.p;
    HIP_CHECK((hipError_t)xmTestBoundLaunch(t, nullptr));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out3, dOut.p, sizeof(int64_t) * 3, hipMemcpyDeviceToHost));
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_bound: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_kat.py): see xm_test_local_kernel (xm_align_kernel.hip) and xm_test_wave_search_kernel (xm_wave_kernel.hip).
int xm_test_local_align(int32_t device, int32_t chain, int32_t mode, const xm_params* p, const uint8_t* query, int32_t query_length, const uint8_t* reference, int32_t reference_length,
                        double max_ins_ext, double max_del_ext, int32_t block_cap, int32_t* blocks, int32_t* num_blocks, double* penalties, int64_t* nodes_put) {
  if (!p || !query || !reference || !blocks || !num_blocks || !penalties) { fail("xm_test_local_align: null argument"); return -1; }
  const bool withBound = mode >= 8;  // mode + 8 (modes 0, 1, 4): the search behind the rejection filter of xm_bound.h; xm_test_bound_counters() says what it did
  if (withBound) mode -= 8;
  if (chain < 0 || chain > 1 || mode < 0 || mode > 4 || (withBound && (mode == 2 || mode == 3)) || (chain == 1 && (mode == 2 || mode == 3)) || query_length < 1 || reference_length < 1 || query_length > 30000 || reference_length > 100000 || block_cap < 1)
  { fail("xm_test_local_align: bad arguments (chain 0: modes 0 LDS slot, 1 HBM, 2 wave search with the search kernel's capacities, 3 with the inline capacities, 4 lane-private form; chain 1: modes 0, 1, 4)"); return -1; }
  try {
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    const Params params = paramsFromC(*p);
    const int cap = block_cap < 256 ? block_cap : 256;
    DevBuf<uint8_t> dq, dr, arena, nodes;
    DevBuf<int32_t> dInts;
    DevBuf<double> dDbls;
    DevBuf<int64_t> dStart;
    DevBuf<int32_t> dLen;
    dq.ensure((size_t)query_length); dr.ensure((size_t)reference_length); dInts.ensure((size_t)8 + 4 * (size_t)cap); dDbls.ensure(2);
    HIP_CHECK(hipMemcpy(dq.p, query, (size_t)query_length, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dr.p, reference, (size_t)reference_length, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dInts.p, 0, sizeof(int32_t) * (8 + 4 * (size_t)cap)));
    HIP_CHECK(hipMemset(dDbls.p, 0, sizeof(double) * 2));
    if (mode == 2 || mode == 3) {
      TestSearch t;
      memset(&t, 0, sizeof(t));
      t.big = mode == 2 ? 1 : 0;
      const int64_t start0 = 0;
      const int32_t len0 = reference_length;
      dStart.ensure(1); dLen.ensure(1);
      HIP_CHECK(hipMemcpy(dStart.p, &start0, 8, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dLen.p, &len0, 4, hipMemcpyHostToDevice));
      t.ix.numContigs = 1; t.ix.refCodes = dr.p; t.ix.contigStart = dStart.p; t.ix.contigLen = dLen.p;
      t.params = params; t.query = dq.p; t.queryLength = query_length; t.referenceLength = reference_length; t.predictedBestOffset = 0; t.confident = 0; t.blockCap = cap;
      t.maxIns = max_ins_ext; t.maxDel = max_del_ext;
      nodes.ensure((size_t)xmTestWaveSearchNodeBytes(t.big));
      t.nodes = nodes.p; t.outInts = dInts.p; t.outDbls = dDbls.p;
      const int rc = xmTestWaveSearchLaunch(t, 0);
      if (rc != 0) throw std::runtime_error(std::string("test search launch: ") + hipGetErrorString((hipError_t)rc));
    } else {
      const int scale = 4;
      const size_t arenaBytes = (size_t)XM_ARENA_KB_DEFAULT * 1024 * scale;
      arena.ensure(arenaBytes);
      nodes.ensure((size_t)XM_PAL_NODES * 4 * sizeof(PNode));
      TestLocalLaunch t{};
      t.chain = chain; t.mode = mode + (withBound ? 8 : 0); t.params = params; t.query = dq.p; t.queryLength = query_length; t.reference = dr.p; t.referenceLength = reference_length;
      t.maxIns = max_ins_ext; t.maxDel = max_del_ext; t.scale = scale; t.arena = arena.p; t.arenaBytes = arenaBytes; t.waveNodes = (PNode*)nodes.p; t.blockCap = cap;
      t.outInts = dInts.p; t.outDbls = dDbls.p;
      HIP_CHECK((hipError_t)xmTestLocalLaunch(t, nullptr));
    }
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<int32_t> ints((size_t)8 + 4 * (size_t)cap);
    double dbls[2];
    HIP_CHECK(hipMemcpy(ints.data(), dInts.p, sizeof(int32_t) * ints.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; i++) g_testBound[i] = ints[(size_t)4 + 4 * (size_t)cap + (size_t)i];
    HIP_CHECK(hipMemcpy(dbls, dDbls.p, sizeof(dbls), hipMemcpyDeviceToHost));
    if (nodes_put) *nodes_put = ints[3];
    const int ok = (mode == 2 || mode == 3) ? ints[0] : (ints[2] != XM_OK ? -1 : ints[0]);
    if (ok < 0) { fail("xm_test_local_align: the search failed with status " + std::to_string(ints[2])); return -1; }
    if (ok == 0) { *num_blocks = 0; return 1; }
    if (ints[1] > cap) { fail("xm_test_local_align: more blocks than block_cap"); return -1; }
    *num_blocks = ints[1];
    memcpy(blocks, ints.data() + 4, sizeof(int32_t) * 4 * (size_t)ints[1]);
    penalties[0] = dbls[0]; penalties[1] = dbls[1];
    return 0;
  } catch (std::exception& e) { fail(std::string("xm_test_local_align: ") + e.what()); return -1; }
}

// Test-only entry (tests/test_gpu_sam.py): xm_sam_format_last's kernels over host-given batch arrays, names, contig names and result streams - no index and
// no alignment.  The host checks what the kernels take on trust from the library's own stages: counts, mates inside codes, offsets that never fall.
int xm_test_sam_format(int32_t device, const xm_test_sam_job* t, xm_sam_text** out) {
  if (!t || !out) return fail("xm_test_sam_format: null argument");
  *out = nullptr;
  try {
    const int64_t nq = t->num_queries;
    if (nq < 0 || t->num_contigs < 0 || t->codes_length < 0) throw std::runtime_error("negative size");
    if (!t->mate_count || !t->mate_offset || !t->mate_length || !t->names || !t->name_off || !t->contig_names || !t->int_off || !t->dbl_off) throw std::runtime_error("null array");
    for (int64_t q = 0; q < nq; q++) {
      if (t->mate_count[q] < 1 || t->mate_count[q] > 2) throw std::runtime_error("mate_count must be 1 or 2");
      for (int m = 0; m < t->mate_count[q]; m++) {
        const int32_t len = t->mate_length[2 * q + m];
        if (len < 0 || t->mate_offset[2 * q + m] < 0 || t->mate_offset[2 * q + m] + len > t->codes_length) throw std::runtime_error("mate outside of codes");
      }
    }
    if (t->int_off[0] != 0 || t->dbl_off[0] != 0) throw std::runtime_error("stream offsets must start at 0");
    for (int64_t q = 0; q < nq; q++) if (t->int_off[q + 1] < t->int_off[q] || t->dbl_off[q + 1] < t->dbl_off[q]) throw std::runtime_error("stream offsets fall");
    const size_t nInts = (size_t)t->int_off[nq], nDbls = (size_t)t->dbl_off[nq];
    if ((nInts && !t->ints) || (nDbls && !t->dbls) || (t->codes_length && !t->codes)) throw std::runtime_error("null array");
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    SamStage g;
    samUploadContigs(g, t->num_contigs, t->contig_names);
    DevBuf<int32_t> dCount, dLength;
    DevBuf<int64_t> dMateOff;
    DevBuf<uint8_t> dCodes;
    dCount.ensure((size_t)nq); dLength.ensure((size_t)nq * 2); dMateOff.ensure((size_t)nq * 2); dCodes.ensure((size_t)t->codes_length);
    if (nq) {
      HIP_CHECK(hipMemcpy(dCount.p, t->mate_count, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dLength.p, t->mate_length, sizeof(int32_t) * (size_t)nq * 2, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dMateOff.p, t->mate_offset, sizeof(int64_t) * (size_t)nq * 2, hipMemcpyHostToDevice));
    }
    if (t->codes_length) HIP_CHECK(hipMemcpy(dCodes.p, t->codes, (size_t)t->codes_length, hipMemcpyHostToDevice));
    const TestStreams up(nq, t->ints, t->dbls, t->int_off, t->dbl_off);
    SamJob job;
    job.batch = xm::SamBatch{nq, dCount.p, dMateOff.p, dLength.p, dCodes.p, nullptr, nullptr};
    job.streams = up.streams(g.numContigs);
    job.contigs = xm::SamContigs{g.numContigs, g.dContigNames.p, g.dContigOff.p};
    const xm_sam_names names{t->names, t->name_off};
    SamBox* box = samFormat(g, job, &names, nullptr);
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_sam_format: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_summary.py): xm_summary_last's kernels over host-given result streams - no index and no alignment.  The host checks what the
// kernels take on trust from the library's own stages: offsets that start at 0 and never fall.  What lies inside a slice may be anything.
int xm_test_summary(int32_t device, int64_t num_queries, int32_t num_contigs, const int32_t* ints, const double* dbls, const int64_t* int_off, const int64_t* dbl_off,
                    int32_t want_unaligned, xm_batch_summary** out) {
  if (!out) return fail("xm_test_summary: null argument");
  *out = nullptr;
  try {
    const int64_t nq = num_queries;
    if (nq < 0 || num_contigs < 0) throw std::runtime_error("negative size");
    if (nq > 0 && (!int_off || !dbl_off)) throw std::runtime_error("null array");
    if (nq > 0 && (int_off[0] != 0 || dbl_off[0] != 0)) throw std::runtime_error("stream offsets must start at 0");
    for (int64_t q = 0; q < nq; q++) if (int_off[q + 1] < int_off[q] || dbl_off[q + 1] < dbl_off[q]) throw std::runtime_error("stream offsets fall");
    const size_t nInts = nq ? (size_t)int_off[nq] : 0, nDbls = nq ? (size_t)dbl_off[nq] : 0;
    if ((nInts && !ints) || (nDbls && !dbls)) throw std::runtime_error("null array");
    SummaryStage g;
    if (nq == 0) { *out = &summaryRun(g, kNoStreams, 0, want_unaligned != 0, nullptr)->pub; return 0; }
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    const TestStreams up(nq, ints, dbls, int_off, dbl_off);
    SummaryBox* box = summaryRun(g, up.streams(num_contigs), nq, want_unaligned != 0, nullptr);
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_summary: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_unaligned.py): xm_unaligned_format_last's kernels over host-given batch arrays, names, qualities, has_qual and the four
// result streams - no index and no alignment.  The host checks what the kernels take on trust from the library's own stages: counts, and offsets that start
// at 0 and never fall.  What lies inside a slice may be anything, and a mate may lie anywhere: the kernels clip their loads to the arrays.
int xm_test_unaligned_format(int32_t device, const xm_test_unaligned_job* t, xm_sam_text** out) {
  if (!t || !out) return fail("xm_test_unaligned_format: null argument");
  *out = nullptr;
  try {
    const int64_t nq = t->num_queries;
    if (nq < 0 || t->num_contigs < 0 || t->codes_length < 0) throw std::runtime_error("negative size");
    UnalignedStage g;
    if (nq == 0) {
      xm::UnalignedBatch none;
      memset(&none, 0, sizeof(none));
      *out = &unalignedFormat(g, none, kNoStreams, nullptr)->pub;
      return 0;
    }
    if (!t->mate_count || !t->mate_offset || !t->mate_length || !t->names || !t->name_off || !t->int_off || !t->dbl_off) throw std::runtime_error("null array");
    const bool withQual = t->has_qual != nullptr;
    if (withQual && (!t->quals || !t->qual_off)) throw std::runtime_error("has_qual without quals and qual_off");
    for (int64_t q = 0; q < nq; q++) if (t->mate_count[q] < 1 || t->mate_count[q] > 2) throw std::runtime_error("mate_count must be 1 or 2");
    const int64_t nameBytes = samCheckNameOffsets(t->name_off, nq);
    int64_t qualBytes = 0;
    if (withQual) {
      if (t->qual_off[0] != 0) throw std::runtime_error("qual_off must start at 0");
      for (int64_t i = 0; i < 2 * nq; i++) if (t->qual_off[i + 1] < t->qual_off[i]) throw std::runtime_error("qual_off falls at entry " + std::to_string(i + 1));
      qualBytes = t->qual_off[2 * nq];
    }
    if (t->int_off[0] != 0 || t->dbl_off[0] != 0) throw std::runtime_error("stream offsets must start at 0");
    for (int64_t q = 0; q < nq; q++) if (t->int_off[q + 1] < t->int_off[q] || t->dbl_off[q + 1] < t->dbl_off[q]) throw std::runtime_error("stream offsets fall");
    const size_t nInts = (size_t)t->int_off[nq], nDbls = (size_t)t->dbl_off[nq];
    if ((nInts && !t->ints) || (nDbls && !t->dbls) || (t->codes_length && !t->codes)) throw std::runtime_error("null array");
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    DevBuf<int32_t> dCount, dLength;
    DevBuf<int64_t> dMateOff, dNameOff, dQualOff;
    DevBuf<uint8_t> dCodes, dHasQual;
    DevBuf<char> dNames, dQuals;
    const size_t slots = (size_t)nq * 2;
    dCount.ensure((size_t)nq); dLength.ensure(slots); dMateOff.ensure(slots); dCodes.ensure((size_t)t->codes_length); dNames.ensure((size_t)nameBytes); dNameOff.ensure(slots + 1);
    HIP_CHECK(hipMemcpy(dCount.p, t->mate_count, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dLength.p, t->mate_length, sizeof(int32_t) * slots, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dMateOff.p, t->mate_offset, sizeof(int64_t) * slots, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dNameOff.p, t->name_off, sizeof(int64_t) * (slots + 1), hipMemcpyHostToDevice));
    if (nameBytes) HIP_CHECK(hipMemcpy(dNames.p, t->names, (size_t)nameBytes, hipMemcpyHostToDevice));
    if (t->codes_length) HIP_CHECK(hipMemcpy(dCodes.p, t->codes, (size_t)t->codes_length, hipMemcpyHostToDevice));
    if (withQual) {
      dQuals.ensure((size_t)qualBytes); dQualOff.ensure(slots + 1); dHasQual.ensure(slots);
      HIP_CHECK(hipMemcpy(dQualOff.p, t->qual_off, sizeof(int64_t) * (slots + 1), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dHasQual.p, t->has_qual, slots, hipMemcpyHostToDevice));
      if (qualBytes) HIP_CHECK(hipMemcpy(dQuals.p, t->quals, (size_t)qualBytes, hipMemcpyHostToDevice));
    }
    const TestStreams up(nq, t->ints, t->dbls, t->int_off, t->dbl_off);
    const xm::UnalignedBatch b{nq, dCount.p, dMateOff.p, dLength.p, dCodes.p, t->codes_length, dNames.p, dNameOff.p, nameBytes,
                               withQual ? dQuals.p : nullptr, withQual ? dQualOff.p : nullptr, withQual ? dHasQual.p : nullptr, qualBytes};
    SamBox* box = unalignedFormat(g, b, up.streams(t->num_contigs), nullptr);
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_unaligned_format: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_refs_count.py): xm_refs_count_last's kernels over host-given result streams - no index and no alignment -, with the sets'
// fingerprints cut to fingerprint_bits bits (64 and more: whole).  The host checks what xm_test_summary checks.
int xm_test_refs_count(int32_t device, int64_t num_queries, int32_t num_contigs, const int32_t* ints, const double* dbls, const int64_t* int_off, const int64_t* dbl_off,
                       int32_t fingerprint_bits, xm_refs_count** out) {
  if (!out) return fail("xm_test_refs_count: null argument");
  *out = nullptr;
  try {
    const int64_t nq = num_queries;
    if (nq < 0 || num_contigs < 0) throw std::runtime_error("negative size");
    if (fingerprint_bits < 1) throw std::runtime_error("fingerprint_bits must be >= 1");
    if (nq > 0 && (!int_off || !dbl_off)) throw std::runtime_error("null array");
    if (nq > 0 && (int_off[0] != 0 || dbl_off[0] != 0)) throw std::runtime_error("stream offsets must start at 0");
    for (int64_t q = 0; q < nq; q++) if (int_off[q + 1] < int_off[q] || dbl_off[q + 1] < dbl_off[q]) throw std::runtime_error("stream offsets fall");
    const size_t nInts = nq ? (size_t)int_off[nq] : 0, nDbls = nq ? (size_t)dbl_off[nq] : 0;
    if ((nInts && !ints) || (nDbls && !dbls)) throw std::runtime_error("null array");
    const int bits = fingerprint_bits > 64 ? 64 : fingerprint_bits;
    RefsStage g;
    if (nq == 0) { *out = &refsRun(g, kNoStreams, 0, bits, nullptr)->pub; return 0; }
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    const TestStreams up(nq, ints, dbls, int_off, dbl_off);
    RefsBox* box = refsRun(g, up.streams(num_contigs), nq, bits, nullptr);
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_refs_count: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_mutations.py): the kernels of xm_pileup_absorb, xm_pileup_call_snps and xm_pileup_judge_indels over host-given counts - no
// index, no alignment and no pile-up; the contigs are their lengths.  With two sets the second is absorbed into the first; rows and verdicts are the first's.
int xm_test_pileup_call(int32_t device, const xm_test_mutations_job* t, xm_snp_calls** out) {
  if (!t || !out) return fail("xm_test_pileup_call: null argument");
  *out = nullptr;
  try {
    if (t->num_contigs < 1 || !t->contig_lengths) throw std::runtime_error("at least one contig is needed");
    if (t->num_sets < 1 || t->num_sets > 2) throw std::runtime_error("num_sets must be 1 or 2");
    if (!t->filter) throw std::runtime_error("null filter");
    if (t->num_candidates < 0 || (t->num_candidates > 0 && (!t->candidates || !t->verdicts))) throw std::runtime_error("candidates without arrays");
    std::vector<int64_t> start((size_t)t->num_contigs);
    long long total = 0;
    for (int c = 0; c < t->num_contigs; c++) {
      if (t->contig_lengths[c] < 1) throw std::runtime_error("a contig without bases");
      start[(size_t)c] = total;
      total += t->contig_lengths[c];
    }
    const bool withMiddle = t->middle[0] != nullptr;
    for (int s = 0; s < t->num_sets; s++) {
      if (!t->depth[s] || !t->alt[s]) throw std::runtime_error("null array");
      if ((t->middle[s] != nullptr) != withMiddle) throw std::runtime_error("every set has a middle depth or none has");
    }
    mutationsCheckCandidates(t->candidates, t->num_candidates, t->contig_lengths, t->num_contigs);
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    const size_t bytes = sizeof(unsigned long long) * (size_t)total;
    DevBuf<unsigned long long> dDepth[2], dAlt[2], dMid[2];
    MutationsCounts counts[2];
    for (int s = 0; s < t->num_sets; s++) {
      dDepth[s].ensure((size_t)total); dAlt[s].ensure((size_t)total * 4);
      HIP_CHECK(hipMemcpy(dDepth[s].p, t->depth[s], bytes, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dAlt[s].p, t->alt[s], bytes * 4, hipMemcpyHostToDevice));
      if (withMiddle) { dMid[s].ensure((size_t)total); HIP_CHECK(hipMemcpy(dMid[s].p, t->middle[s], bytes, hipMemcpyHostToDevice)); }
      counts[s] = MutationsCounts{dDepth[s].p, dAlt[s].p, withMiddle ? dMid[s].p : nullptr, total};
    }
    MutationsStage g;
    if (t->num_sets == 2) { mutationsAbsorb(counts[0], counts[1], nullptr); HIP_CHECK(hipDeviceSynchronize()); }
    const xm::MutationFilter f = mutationsFilter(t->filter);
    SnpBox* box = mutationsSelect(g, counts[0], start.data(), t->contig_lengths, t->num_contigs, f, nullptr);
    try {
      if (t->num_candidates > 0) mutationsJudge(g, counts[0], start.data(), t->contig_lengths, t->num_contigs, f, t->candidates, t->num_candidates, t->verdicts, nullptr);
      for (int s = 0; s < t->num_sets; s++) {
        if (!t->read_back[s]) continue;
        HIP_CHECK(hipMemcpy(t->read_back[s], dDepth[s].p, bytes, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(t->read_back[s] + total, dAlt[s].p, bytes * 4, hipMemcpyDeviceToHost));
        if (withMiddle) HIP_CHECK(hipMemcpy(t->read_back[s] + total * 5, dMid[s].p, bytes, hipMemcpyDeviceToHost));
      }
    } catch (...) {
      freeSnpBox(box);
      throw;
    }
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_pileup_call: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_pileup_text.py): the three stages of xm_pileup_text.h - what xm_pileup_add_last runs with kept text - over host-given events
// and batch arrays; no index, no alignment, no pile-up kernel (so the total is read from the offsets).  The host checks what the kernels take on trust from
// the library's own stages: mates inside codes.  The events may hold anything.  launches: kernels launched (4 without text to gather, 5 with; 0 for no events).
int xm_test_pileup_text(int32_t device, const xm_test_pileup_job* t, int64_t* text_off, char* text, int64_t text_cap, int32_t* launches) {
  if (!t || !text_off) return fail("xm_test_pileup_text: null argument");
  try {
    const int64_t nq = t->num_queries, n = t->num_events;
    if (nq < 0 || n < 0 || t->codes_length < 0 || text_cap < 0) throw std::runtime_error("negative size");
    if ((nq && (!t->mate_offset || !t->mate_length)) || (t->codes_length && !t->codes) || (n && !t->events)) throw std::runtime_error("null array");
    for (int64_t k = 0; k < 2 * nq; k++) {
      const int32_t len = t->mate_length[k];
      if (len < 0 || t->mate_offset[k] < 0 || t->mate_offset[k] + len > t->codes_length) throw std::runtime_error("mate outside of codes");
    }
    if (launches) *launches = 0;
    text_off[0] = 0;
    if (n == 0) return 0;
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    DevBuf<int32_t> dLength;
    DevBuf<int64_t> dMateOff;
    DevBuf<uint8_t> dCodes;
    DevBuf<long long> dEvents;
    dLength.ensure((size_t)nq * 2); dMateOff.ensure((size_t)nq * 2); dCodes.ensure((size_t)t->codes_length); dEvents.ensure((size_t)n * 8);
    if (nq) {
      HIP_CHECK(hipMemcpy(dLength.p, t->mate_length, sizeof(int32_t) * (size_t)nq * 2, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dMateOff.p, t->mate_offset, sizeof(int64_t) * (size_t)nq * 2, hipMemcpyHostToDevice));
    }
    if (t->codes_length) HIP_CHECK(hipMemcpy(dCodes.p, t->codes, (size_t)t->codes_length, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dEvents.p, t->events, sizeof(int64_t) * (size_t)n * 8, hipMemcpyHostToDevice));
    PileupTextStage stage;
    const PileupTextJob job{dEvents.p, (long long)n, (long long)t->query_base, (long long)nq, dMateOff.p, dLength.p, dCodes.p};
    stage.offsets(job, nullptr);
    HIP_CHECK(hipMemcpy(text_off, stage.dOff.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    if (launches) *launches = 4;
    const int64_t total = text_off[n];
    if (total > text_cap) throw std::runtime_error("the text takes " + std::to_string(total) + " bytes");
    if (total > 0) {
      if (!text) throw std::runtime_error("null array");
      stage.gather(job, total, nullptr);
      if (launches) *launches = 5;
      HIP_CHECK(hipMemcpy(text, stage.dText.p, (size_t)total, hipMemcpyDeviceToHost));
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_pileup_text: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_indel_groups.py): the fold of xm_pileup_add_last with grouping on, the absorb of xm_pileup_absorb and the unjudged end of
// xm_pileup_call_indels over host-given events and text - no index, no alignment and no pile-up.  The events may hold anything; the host checks the offsets.
int xm_test_pileup_group(int32_t device, xm_test_group_job* t, xm_indel_calls** out) {
  if (!t || !out) return fail("xm_test_pileup_group: null argument");
  *out = nullptr;
  try {
    if (t->fingerprint_bits < 1) throw std::runtime_error("fingerprint_bits must be >= 1");
    if (t->initial_capacity < 0 || t->left_cap < 0 || t->left_text_cap < 0) throw std::runtime_error("negative size");
    if (t->num_calls[0] < 0 || t->num_calls[1] < 0 || (t->num_calls[0] && !t->calls[0]) || (t->num_calls[1] && !t->calls[1])) throw std::runtime_error("calls without arrays");
    for (int set = 0; set < 2; set++)
      for (int k = 0; k < t->num_calls[set]; k++) {
        const xm_test_group_call& c = t->calls[set][k];
        if (c.num_events < 0) throw std::runtime_error("negative size");
        if (c.num_events == 0) continue;
        if (!c.events || !c.text_off) throw std::runtime_error("null array");
        if (c.text_off[0] != 0) throw std::runtime_error("text offsets must start at 0");
        for (int64_t i = 0; i < c.num_events; i++) if (c.text_off[i + 1] < c.text_off[i]) throw std::runtime_error("text offsets fall");
        if (c.text_off[c.num_events] > 0 && !c.text) throw std::runtime_error("null array");
      }
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    IGroupsStage stage[2];
    std::vector<long long> events;
    std::vector<int64_t> textOff;
    std::vector<char> text;
    std::vector<int32_t> callOf;
    const IGroupsLeft left{&events, &textOff, &text};
    int ordinal = 0;
    for (int set = 0; set < 2; set++) {
      stage[set].bits = t->fingerprint_bits > 64 ? 64 : t->fingerprint_bits;
      stage[set].leastCap = (unsigned long long)t->initial_capacity;
      for (int k = 0; k < t->num_calls[set]; k++, ordinal++) {
        const xm_test_group_call& c = t->calls[set][k];
        const int64_t n = c.num_events;
        if (n == 0) continue;
        const int64_t bytes = c.text_off[n];
        DevBuf<long long> dEvents;
        DevBuf<int64_t> dOff;
        DevBuf<char> dText;
        dEvents.ensure((size_t)n * 8); dOff.ensure((size_t)n + 1); dText.ensure((size_t)bytes + 1);
        HIP_CHECK(hipMemcpy(dEvents.p, c.events, sizeof(int64_t) * (size_t)n * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dOff.p, c.text_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
        if (bytes) HIP_CHECK(hipMemcpy(dText.p, c.text, (size_t)bytes, hipMemcpyHostToDevice));
        stage[set].reserve(n, bytes, nullptr);
        const long long nLeft = stage[set].fold(IGroupsItems{dEvents.p, dOff.p, dText.p, nullptr, nullptr, n}, nullptr, left);
        callOf.insert(callOf.end(), (size_t)nLeft, (int32_t)ordinal);
        HIP_CHECK(hipDeviceSynchronize());
      }
    }
    if (t->num_calls[1] > 0) {
      const size_t before = events.size() / 8;
      igroupsAbsorb(stage[0], current, stage[1], current, left);
      callOf.insert(callOf.end(), events.size() / 8 - before, (int32_t)ordinal);
      if (stage[1].groups != 0) throw std::runtime_error("internal error: the absorbed table is not empty");
    }
    const int64_t nLeft = (int64_t)(events.size() / 8), leftBytes = (int64_t)text.size();
    if (nLeft > t->left_cap || leftBytes > t->left_text_cap) throw std::runtime_error("the left-overs take " + std::to_string(nLeft) + " events and " + std::to_string(leftBytes) + " bytes");
    if (nLeft && (!t->left_events || !t->left_call || !t->left_text_off || (leftBytes && !t->left_text))) throw std::runtime_error("null array");
    t->num_left = nLeft;
    if (nLeft) {
      memcpy(t->left_events, events.data(), sizeof(long long) * events.size());
      memcpy(t->left_call, callOf.data(), sizeof(int32_t) * callOf.size());
      memcpy(t->left_text_off, textOff.data(), sizeof(int64_t) * ((size_t)nLeft + 1));
      if (leftBytes) memcpy(t->left_text, text.data(), (size_t)leftBytes);
    } else if (t->left_text_off) {
      t->left_text_off[0] = 0;
    }
    t->grows[0] = stage[0].tableGrows; t->grows[1] = stage[0].recordGrows; t->grows[2] = stage[0].arenaGrows;
    MutationsStage m;
    IndelBox* box = igroupsCall(stage[0], m, nullptr, nullptr, nullptr, 0, nullptr, nullptr);
    box->pub.left_over = nLeft;
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_pileup_group: ") + e.what()); }
}

}  // extern "C"

namespace {

// xm_test_scan's compaction: the kept items in ascending order, as a scan of the mask
struct ScanTestKept {
  static constexpr int N = 1;
  long long n;
  const uint8_t* keep;
  int64_t* list; long long* total;
  __device__ long long count() const { return n; }
  __device__ void lens(long long i, long long v[1]) const { v[0] = keep[i] ? 1 : 0; }
  __device__ void put(long long i, const long long at[1]) const { if (keep[i]) list[at[0]] = i; }
  __device__ void totals(const long long t[1]) const { total[0] = t[0]; }
};

// the buffers of xm_test_scan, kept from call to call (a scan's block sums outlive the call that sized them everywhere else, too); never destroyed, as g_pinned
struct ScanTestStage {
  std::mutex mu;
  int device = -1;
  DevBuf<long long> dLens, dBlockSums, dTotal;
  DevBuf<int64_t> dOff, dKept;
  DevBuf<uint8_t> dKeep;
};
ScanTestStage* g_scanTest = new ScanTestStage();

template <int CH>
void scanTestOffsets(ScanTestStage& g, long long n) {
  XmOffsets<long long, CH> items;
  items.n = n;
  for (int j = 0; j < CH; j++) { items.len[j] = g.dLens.p + (size_t)j * (size_t)n; items.off[j] = g.dOff.p + (size_t)j * ((size_t)n + 1); }
  xmScan(items, n, g.dBlockSums, nullptr);
}

}  // namespace

extern "C" {

// Test-only entry (tests/test_gpu_scan.py): the scan of xm_scan.h alone.  lens: `channels` (1, 2 or 3) arrays of n lengths one behind the other; offsets gets
// the n + 1 exclusive sums of each the same way.  keep (may be NULL): n bytes, 0 or 1 - kept[0 .. *num_kept) then gets the indices of the kept items in
// ascending order, by a second scan over the mask with the same block sums.
int xm_test_scan(int32_t device, int32_t channels, int64_t n, const int64_t* lens, const uint8_t* keep, int64_t* offsets, int64_t* kept, int64_t* num_kept) {
  if (channels < 1 || channels > 3 || n < 0 || !offsets || (n > 0 && !lens) || (keep && (!kept || !num_kept))) return fail("xm_test_scan: bad arguments");
  try {
    ScanTestStage& g = *g_scanTest;
    std::lock_guard<std::mutex> lock(g.mu);
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    int current = 0;
    HIP_CHECK(hipGetDevice(&current));
    if (g.device != current) {  // (buffers of another GPU are of no use)
      g.dLens.release(); g.dBlockSums.release(); g.dTotal.release(); g.dOff.release(); g.dKept.release(); g.dKeep.release();
      g.device = current;
    }
    const size_t nLens = (size_t)channels * (size_t)n, nOff = (size_t)channels * ((size_t)n + 1);
    g.dLens.ensure(nLens); g.dOff.ensure(nOff);
    if (nLens) HIP_CHECK(hipMemcpy(g.dLens.p, lens, sizeof(int64_t) * nLens, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(g.dOff.p, 0xFF, sizeof(int64_t) * nOff));  // (an offset the scan does not write shows)
    if (channels == 1) scanTestOffsets<1>(g, n);
    else if (channels == 2) scanTestOffsets<2>(g, n);
    else scanTestOffsets<3>(g, n);
    if (keep) {
      g.dKeep.ensure((size_t)n); g.dKept.ensure((size_t)n); g.dTotal.ensure(1);
      if (n) HIP_CHECK(hipMemcpy(g.dKeep.p, keep, (size_t)n, hipMemcpyHostToDevice));
      if (n) HIP_CHECK(hipMemset(g.dKept.p, 0xFF, sizeof(int64_t) * (size_t)n));
      xmScan(ScanTestKept{n, g.dKeep.p, g.dKept.p, g.dTotal.p}, n, g.dBlockSums, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(offsets, g.dOff.p, sizeof(int64_t) * nOff, hipMemcpyDeviceToHost));
    if (keep) {
      long long total = 0;
      HIP_CHECK(hipMemcpy(&total, g.dTotal.p, sizeof(total), hipMemcpyDeviceToHost));
      if (total < 0 || total > n) throw std::runtime_error("the scan kept " + std::to_string(total) + " of " + std::to_string(n) + " items");
      if (total) HIP_CHECK(hipMemcpy(kept, g.dKept.p, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost));
      *num_kept = total;
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_scan: ") + e.what()); }
}

// Test-only entry (tests/test_gpu_sam.py): Double.toString of xm_sam_rules.h run by the device on n values; out24 gets 24 bytes a value, len the lengths.
int xm_test_format_doubles(int32_t device, int64_t n, const double* x, char* out24, int32_t* len) {
  if (n < 0 || (n > 0 && (!x || !out24 || !len))) return fail("xm_test_format_doubles: bad arguments");
  try {
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    if (n == 0) return 0;
    DevBuf<double> dX;
    DevBuf<char> dOut;
    DevBuf<int32_t> dLen;
    dX.ensure((size_t)n); dOut.ensure((size_t)n * xm::XM_SAM_DOUBLE_BYTES); dLen.ensure((size_t)n);
    HIP_CHECK(hipMemcpy(dX.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(xm_sam_doubles_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (long long)n, (const double*)dX.p, dOut.p, dLen.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out24, dOut.p, (size_t)n * xm::XM_SAM_DOUBLE_BYTES, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(len, dLen.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_test_format_doubles: ") + e.what()); }
}

}  // extern "C"
