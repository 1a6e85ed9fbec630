// The seed-probe and random-gather micro-benchmarks of libxmapper_hip.so (included once, by xm_capi.hip, behind xm_index): their kernels and
// the two C entries that launch them.
#pragma once

namespace {

// Where a probe's positions go: the 64 probes i = 64 c ... 64 c + 63 (the lanes of one wavefront) write theirs one behind the other, in probe order, from
// out_positions[64 c max_per_probe] on - whole lines leave for HBM, and only as many bytes as there are positions (rows of max_per_probe slots cost the
// memory 56 bytes a probe at 7 slots, of which a genome's buckets fill 12; a row per position index, written only where a bucket has that many, is holes
// in every line, and a partly written line costs a read besides the write).  The reader finds probe i's positions behind those of the probes before it
// in its chunk: offsets are the running sum of min(max(counts, 0), max_per_probe) over the chunk.  Returns this lane's first slot.
__device__ __forceinline__ long long xmProbeSlot(long long i, int m, int maxPerProbe) {
  // exclusive prefix sum of m (0 ... 7: three bits) over the lanes of the wave
  const unsigned long long b0 = __ballot(m & 1), b1 = __ballot(m & 2), b2 = __ballot(m & 4), b3 = __ballot(m & 8);
  const unsigned long long below = (1ull << (threadIdx.x & 63u)) - 1ull;
  const int before = __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below) + 8 * __popcll(b3 & below);
  return (i & ~63ll) * (long long)maxPerProbe + before;
}

// PackedMap.getNumMatchesLowerBound + PackedMap.get for a batch of (used length, key): one lane per probe.
__global__ void __launch_bounds__(256) xm_seed_probe_kernel(IndexView ix, long long n, const int32_t* usedLength, const int32_t* keys, int maxPerProbe,
                                                            int32_t* counts, int64_t* outPositions) {
  // (the probe through the CSR arrays - two adjacent offsets, then the positions: what an index without bucket lines offers)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const int used = live ? usedLength[i] : -1;
  const bool ok = live && used >= 0 && used <= ix.maxHashedLength;
  int count = -2;
  int64_t first = 0;
  if (ok) {
    const Table* t = &ix.tables[used];
    const uint32_t k = packedKey(t, keys[i]);
    const uint32_t* off = ix.bucketOff + t->offBase + k;
    const uint32_t o0 = off[0], o1 = off[1];
    count = (o0 & XM_OVERFULL) ? -1 : (int)((o1 & ~XM_OVERFULL) - (o0 & ~XM_OVERFULL));
    if (count > t->maxCount) count = -1;
    first = t->posBase + (int64_t)(o0 & ~XM_OVERFULL);
  }
  const int m = (count > 0 && maxPerProbe > 0) ? (count < maxPerProbe ? count : maxPerProbe) : 0;
  const long long slot = xmProbeSlot(i, m, maxPerProbe);
  if (!live) return;
  counts[i] = count;
  for (int j = 0; j < m; j++) outPositions[slot + j] = ix.posIs64 ? (int64_t)ix.positions64[first + j] : (int64_t)ix.positions32[first + j];
}

// The same bulk probe over bucket lines with several probes in flight per lane (round 5; it replaces the group-of-lanes form of round 2, which ran at half of this
// GPU's random-sector rate): a probe's chain - (length, key) -> table descriptor -> key mod capacity -> line - is short but dependent, so what the rate
// needs is many chains at a time.  A lane takes XM_PROBES_PER_LANE probes a whole launch apart (coalesced reads of the inputs and writes of the counts), takes
// the table descriptors from LDS (the block copies them there once: no trip to memory between the inputs and the line), and has asked for all its lines
// before it looks at the first.  64-bit lines: the whole 64-byte line as four 16-byte loads; 32-bit lines: two.  Header only (maxPerProbe == 0): the first
// 16 bytes.  Buckets with more than XM_LINE_SLOTS positions (1.4 % of a genome-like index) read the CSR arrays behind that.
constexpr int XM_PROBES_PER_LANE = 4;
constexpr int XM_PROBE_LDS_TABLES = 512;
template <bool W64>
__global__ void __launch_bounds__(256) xm_seed_probe_lines_kernel(IndexView ix, long long n, const int32_t* usedLength, const int32_t* keys, int maxPerProbe,
                                                                  int32_t* counts, int64_t* outPositions) {
  __shared__ Table sTables[XM_PROBE_LDS_TABLES];
  const int nTables = ix.maxHashedLength + 1;
  const bool inLds = nTables <= XM_PROBE_LDS_TABLES;
  if (inLds) {
    for (int t = (int)threadIdx.x; t < nTables; t += (int)blockDim.x) sTables[t] = ix.tables[t];
    __syncthreads();
  }
  const long long lanes = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int used[XM_PROBES_PER_LANE], key[XM_PROBES_PER_LANE];
#pragma unroll
  for (int p = 0; p < XM_PROBES_PER_LANE; p++) {
    const long long i = tid + (long long)p * lanes;
    used[p] = i < n ? usedLength[i] : -1;
    key[p] = i < n ? keys[i] : 0;
  }
  Table tb[XM_PROBES_PER_LANE];
  uint32_t k[XM_PROBES_PER_LANE];
  typedef typename std::conditional<W64, ulonglong2, uint4>::type Vec;   // 16 bytes of a line
  constexpr int NV = W64 ? 4 : 2;
  Vec v[XM_PROBES_PER_LANE][NV];
#pragma unroll
  for (int p = 0; p < XM_PROBES_PER_LANE; p++) {
    const bool ok = used[p] >= 0 && used[p] <= ix.maxHashedLength;
    tb[p] = inLds ? sTables[ok ? used[p] : 0] : ix.tables[ok ? used[p] : 0];
    k[p] = packedKey(&tb[p], key[p]);
    const Vec* lp = W64 ? (const Vec*)(ix.lines64 + (tb[p].offBase + k[p]) * 8) : (const Vec*)(ix.lines32 + (tb[p].offBase + k[p]) * 8);
    if (ok) v[p][0] = lp[0];
  }
  // the rest of a line only where its positions are wanted: the first 16 bytes hold the count and three positions (one with 64-bit positions), and a
  // request costs the memory pipeline the same whether it brings 16 bytes of a new sector or the next 16 of the one before
  int cnt[XM_PROBES_PER_LANE];
#pragma unroll
  for (int p = 0; p < XM_PROBES_PER_LANE; p++) {
    const bool ok = used[p] >= 0 && used[p] <= ix.maxHashedLength;
    const uint32_t h = W64 ? (uint32_t)((const unsigned long long*)&v[p][0])[0] : ((const uint32_t*)&v[p][0])[0];
    int count = (h & XM_OVERFULL) ? -1 : (int)h;
    if (ok && count > tb[p].maxCount) count = -1;
    cnt[p] = ok ? count : -2;
    const int want = (maxPerProbe > 0 && count > 0 && count <= XM_LINE_SLOTS) ? (count < maxPerProbe ? count : maxPerProbe) : 0;   // positions to take from the line
    const Vec* lp = W64 ? (const Vec*)(ix.lines64 + (tb[p].offBase + k[p]) * 8) : (const Vec*)(ix.lines32 + (tb[p].offBase + k[p]) * 8);
#pragma unroll
    for (int q = 1; q < NV; q++) if (ok && 1 + want > q * (W64 ? 2 : 4)) v[p][q] = lp[q];
  }
#pragma unroll
  for (int p = 0; p < XM_PROBES_PER_LANE; p++) {
    const long long i = tid + (long long)p * lanes;
    const int count = cnt[p];
    const int m = (i < n && count > 0 && maxPerProbe > 0) ? (count < maxPerProbe ? count : maxPerProbe) : 0;
    const long long slot = xmProbeSlot(i, m, maxPerProbe);  // (every lane of the wave: the lanes' probes of one p are 64 consecutive ones)
    if (i >= n) continue;
    counts[i] = count;
    if (m == 0) continue;
    if (count <= XM_LINE_SLOTS) {
#pragma unroll
      for (int j = 0; j < XM_LINE_SLOTS; j++) {
        if (j < m) outPositions[slot + j] = W64 ? (int64_t)((const unsigned long long*)&v[p][0])[1 + j] : (int64_t)((const uint32_t*)&v[p][0])[1 + j];
      }
      continue;
    }
    const int64_t first = tb[p].posBase + (int64_t)(ix.bucketOff[tb[p].offBase + k[p]] & ~XM_OVERFULL);
    for (int j = 0; j < m; j++) outPositions[slot + j] = ix.posIs64 ? (int64_t)ix.positions64[first + j] : (int64_t)ix.positions32[first + j];
  }
}

// Measurement helper: one random 64-byte sector per access out of a table far larger than the caches, 16 bytes of it read.
// The sectors/s this reaches is the ceiling a hash-probe kernel (one 8-byte bucket header per probe) can be held against.
__global__ void __launch_bounds__(256) xm_random_gather_kernel(const uint4* table, unsigned long long nSectors, long long nAccesses, int perThread, unsigned long long seed,
                                                               unsigned int* sink) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (int k = 0; k < perThread; k++) {
    long long a = t * perThread + k;
    if (a >= nAccesses) break;
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(a + 1);  // SplitMix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uint4 v = table[(z % nSectors) * 4];
    acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
  }
  if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) sink[0] = acc.x;  // keeps the loads alive
}

}  // namespace

extern "C" {

int xm_seed_probe_packed(xm_index* idx, int64_t n, const int32_t* usedLength, const int32_t* keys, int32_t maxPerProbe, int32_t* counts, int64_t* outPositions, double* kernelMs) {
  if (!idx || idx->hostOnly) return fail("xm_seed_probe_packed: needs a device-resident index");
  if (maxPerProbe < 0 || maxPerProbe > 15) return fail("xm_seed_probe_packed: max_per_probe must be 0 ... 15");
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    HIP_CHECK(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    DevBuf<int32_t> dUsed, dKeys, dCounts;
    DevBuf<int64_t> dPos;
    dUsed.ensure((size_t)n); dKeys.ensure((size_t)n); dCounts.ensure((size_t)n); dPos.ensure((size_t)n * (size_t)(maxPerProbe > 0 ? maxPerProbe : 1));
    HIP_CHECK(hipMemcpyAsync(dUsed.p, usedLength, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dKeys.p, keys, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    int block = 256;
    int grid = (int)((n + block - 1) / block);
    HIP_CHECK(hipEventRecord(idx->ev0, s));
    std::shared_lock<std::shared_mutex> tablesInUse(idx->dt->rw);
    IndexView view = idx->dt->view;
    if (envInt("XM_PROBE_NO_LINES", 0) != 0) { view.lines32 = nullptr; view.lines64 = nullptr; }  // measurement: the CSR probe (two dependent accesses) on the same index
    const unsigned batched = (unsigned)((n + (long long)block * XM_PROBES_PER_LANE - 1) / ((long long)block * XM_PROBES_PER_LANE));
    if (n > 0 && view.lines64) hipLaunchKernelGGL((xm_seed_probe_lines_kernel<true>), dim3(batched), dim3(block), 0, s, view, (long long)n, dUsed.p, dKeys.p, (int)maxPerProbe, dCounts.p, dPos.p);
    else if (n > 0 && view.lines32) hipLaunchKernelGGL((xm_seed_probe_lines_kernel<false>), dim3(batched), dim3(block), 0, s, view, (long long)n, dUsed.p, dKeys.p, (int)maxPerProbe, dCounts.p, dPos.p);
    else if (n > 0) hipLaunchKernelGGL(xm_seed_probe_kernel, dim3(grid), dim3(block), 0, s, view, (long long)n, dUsed.p, dKeys.p, (int)maxPerProbe, dCounts.p, dPos.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(idx->ev1, s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, idx->ev0, idx->ev1));
    if (kernelMs) *kernelMs = ms;
    HIP_CHECK(hipMemcpy(counts, dCounts.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (outPositions && maxPerProbe > 0) HIP_CHECK(hipMemcpy(outPositions, dPos.p, sizeof(int64_t) * (size_t)n * (size_t)maxPerProbe, hipMemcpyDeviceToHost));
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_seed_probe_packed: ") + e.what()); }
}

int xm_measure_random_gather(int device, int64_t table_bytes, int64_t accesses, double* kernel_ms) {
  try {
    HIP_CHECK(hipSetDevice(device));
    if (table_bytes < 4096 || accesses < 1) return fail("xm_measure_random_gather: bad arguments");
    DevBuf<uint4> table;
    DevBuf<unsigned int> sink;
    const size_t nSectors = (size_t)table_bytes / 64;
    table.ensure(nSectors * 4);
    sink.ensure(1);
    HIP_CHECK(hipMemset(table.p, 0, nSectors * 64));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
    const int perThread = 4;
    const long long threads = (accesses + perThread - 1) / perThread;
    float best = 0;
    for (int rep = 0; rep < 3; rep++) {  // first repetition warms up
      HIP_CHECK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(xm_random_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, table.p, (unsigned long long)nSectors, (long long)accesses, perThread,
                         0x5EED0000ull + rep, sink.p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(e1, 0));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (rep > 0 && (best == 0 || ms < best)) best = ms;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (kernel_ms) *kernel_ms = best;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_measure_random_gather: ") + e.what()); }
}

}  // extern "C"
