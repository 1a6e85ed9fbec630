// The test-only entries of libxmapper_hip.so (included once, by xm_capi.hip): components of the align kernel run alone on given inputs.  Buffers and the
// error contract are here; the kernels stand behind the align kernel in xm_align_kernel.hip (TestLocalLaunch, TestBoundLaunch: xm_kernel_common.h).
#pragma once

extern "C" {

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

}  // extern "C"
