// Exclusive prefix sums in item order (included once, by xm_capi.hip): the one statement of the offset scan every on-GPU output stage uses, and of the two
// block-level loops inside it.  Three kernels, separate launches, because no launch reads what another workgroup of the same launch wrote (the per-XCD L2s
// are not coherent):
//   sums    xm_scan_sums_kernel    16 items a thread, 4096 a block: the block's sums of the items' N lengths -> blockSums[N * block + j]
//   blocks  xm_scan_blocks_kernel  one thread walks the block sums (a million items are 245 blocks), leaves their exclusive sums in place and hands the
//                                  totals to Items::totals
//   place   xm_scan_place_kernel   the block's items again: every item's N offsets -> Items::put, in item order within a thread
// What is summed and where the offsets go is the consumer's Items, a small named struct passed by value (a kernel's name in a trace is the name of its Items):
//   static constexpr int N                                  the lengths of an item: 1, 2 or 3
//   __device__ long long count() const                      the items; the kernels look at no item behind it
//   __device__ void lens(long long i, long long v[N]) const
//   __device__ void put(long long i, const long long off[N]) const    free to store nothing (a compaction) or to scatter; its capacity checks are its own
//   __device__ void totals(const long long t[N]) const      run by the one thread of the blocks kernel: off[n], control words
// The host's side is xmScan (nothing waits, nothing is allocated once blockSums is large enough), or its two halves where the host reads a total in between.
#pragma once
#include "xm_device_rt.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

// (the edges this gives - 16 per thread, 256 per gather block, 4096 per scan block - are walked by tests/test_gpu_scan.py and, through the result stage, by
// tests/test_gpu_result_stage.py)
constexpr int XM_SCAN_PER_THREAD = 16;
constexpr int XM_SCAN_PER_BLOCK = 256 * XM_SCAN_PER_THREAD;

// The two loops over the 256 threads of a block, N values a thread, in the caller's __shared__ T sh[N][256].
// the tree sum: a[] becomes the block's sums, in every thread
template <typename T, int N>
__device__ __forceinline__ void xmBlockSum(T (&a)[N], T (*sh)[256]) {
  for (int j = 0; j < N; j++) sh[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) for (int j = 0; j < N; j++) sh[j][threadIdx.x] += sh[j][threadIdx.x + d];
    __syncthreads();
  }
  for (int j = 0; j < N; j++) a[j] = sh[j][0];
}
// the inclusive Hillis-Steele scan: a[] becomes the sums of the threads up to and including this one; sh[j][255] is then the block's sum
template <typename T, int N>
__device__ __forceinline__ void xmBlockScan(T (&a)[N], T (*sh)[256]) {
  for (int j = 0; j < N; j++) sh[j][threadIdx.x] = a[j];
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    T x[N];
    for (int j = 0; j < N; j++) x[j] = (int)threadIdx.x >= d ? sh[j][threadIdx.x - d] : T(0);
    __syncthreads();
    for (int j = 0; j < N; j++) sh[j][threadIdx.x] += x[j];
    __syncthreads();
  }
  for (int j = 0; j < N; j++) a[j] = sh[j][threadIdx.x];
}

// the sums of the thread's 16 items
template <class Items>
__device__ __forceinline__ void xmScanThreadSums(const Items& items, long long n, long long base, long long (&a)[Items::N]) {
  for (int j = 0; j < Items::N; j++) a[j] = 0;
  for (int k = 0; k < XM_SCAN_PER_THREAD; k++) if (base + k < n) {
    long long v[Items::N];
    items.lens(base + k, v);
    for (int j = 0; j < Items::N; j++) a[j] += v[j];
  }
}

template <class Items>
__global__ void __launch_bounds__(256) xm_scan_sums_kernel(Items items, long long* blockSums) {
  __shared__ long long sh[Items::N][256];
  const long long base = (long long)blockIdx.x * XM_SCAN_PER_BLOCK + (long long)threadIdx.x * XM_SCAN_PER_THREAD;
  long long a[Items::N];
  xmScanThreadSums(items, items.count(), base, a);
  xmBlockSum(a, sh);
  if (threadIdx.x == 0) for (int j = 0; j < Items::N; j++) blockSums[Items::N * (long long)blockIdx.x + j] = a[j];
}

template <class Items>
__global__ void xm_scan_blocks_kernel(Items items, long long nBlocks, long long* blockSums) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long run[Items::N];
  for (int j = 0; j < Items::N; j++) run[j] = 0;
  for (long long i = 0; i < nBlocks; i++)
    for (int j = 0; j < Items::N; j++) { const long long x = blockSums[Items::N * i + j]; blockSums[Items::N * i + j] = run[j]; run[j] += x; }
  items.totals(run);
}

// stride: the lengths the sums pass took per item (more than N where only the first N offsets are placed)
template <class Items>
__global__ void __launch_bounds__(256) xm_scan_place_kernel(Items items, const long long* blockSums, int stride) {
  __shared__ long long sh[Items::N][256];
  const long long n = items.count();
  const long long base = (long long)blockIdx.x * XM_SCAN_PER_BLOCK + (long long)threadIdx.x * XM_SCAN_PER_THREAD;
  long long a[Items::N], off[Items::N];
  xmScanThreadSums(items, n, base, a);
  for (int j = 0; j < Items::N; j++) off[j] = a[j];
  xmBlockScan(off, sh);
  for (int j = 0; j < Items::N; j++) off[j] += blockSums[stride * (long long)blockIdx.x + j] - a[j];  // (inclusive -> exclusive)
  for (int k = 0; k < XM_SCAN_PER_THREAD; k++) if (base + k < n) {
    long long v[Items::N];
    items.lens(base + k, v);
    items.put(base + k, off);
    for (int j = 0; j < Items::N; j++) off[j] += v[j];
  }
}

// the blocks of a scan of n items, and the entries of blockSums it takes with `channels` lengths an item (for a caller that sizes its buffers before it takes a
// stream: a buffer that grows frees the old one, which waits for the device)
constexpr long long xmScanBlocks(long long n) { return (n + XM_SCAN_PER_BLOCK - 1) / XM_SCAN_PER_BLOCK; }
constexpr size_t xmScanSums(long long n, int channels) { return (size_t)(channels * xmScanBlocks(n)); }

// The first two launches, enqueued on s: behind them Items::totals has run.  n: at least Items::count() (it sizes the grid).  For n == 0 only the blocks
// kernel is launched - the totals are still written, and no grid is ever empty.
template <class Items>
void xmScanTotals(const Items& items, long long n, DevBuf<long long>& blockSums, hipStream_t s) {
  const long long nBlocks = xmScanBlocks(n);
  blockSums.ensure(xmScanSums(n, Items::N));
  if (nBlocks > 0) hipLaunchKernelGGL(xm_scan_sums_kernel<Items>, dim3((unsigned)nBlocks), dim3(256), 0, s, items, blockSums.p);
  hipLaunchKernelGGL(xm_scan_blocks_kernel<Items>, dim3(1), dim3(64), 0, s, items, nBlocks, blockSums.p);
  HIP_CHECK(hipGetLastError());
}
// The third launch, behind xmScanTotals on the same stream with the same n and blockSums (sumsN: the N of the Items the totals were taken with).
template <class Items>
void xmScanPlace(const Items& items, long long n, const DevBuf<long long>& blockSums, hipStream_t s, int sumsN = Items::N) {
  const long long nBlocks = xmScanBlocks(n);
  if (nBlocks > 0) hipLaunchKernelGGL(xm_scan_place_kernel<Items>, dim3((unsigned)nBlocks), dim3(256), 0, s, items, (const long long*)blockSums.p, sumsN);
  HIP_CHECK(hipGetLastError());
}
template <class Items>
void xmScan(const Items& items, long long n, DevBuf<long long>& blockSums, hipStream_t s) {
  xmScanTotals(items, n, blockSums, s);
  xmScanPlace(items, n, blockSums, s);
}

// The plain Items: CH arrays of lengths (int32_t or long long), an offset array of n + 1 entries for each.
template <typename T, int CH>
struct XmOffsets {
  static constexpr int N = CH;
  long long n;
  const T* len[CH];
  int64_t* off[CH];
  __device__ long long count() const { return n; }
  __device__ void lens(long long i, long long v[CH]) const { for (int j = 0; j < CH; j++) v[j] = len[j][i]; }
  __device__ void put(long long i, const long long o[CH]) const { for (int j = 0; j < CH; j++) off[j][i] = o[j]; }
  __device__ void totals(const long long t[CH]) const { for (int j = 0; j < CH; j++) off[j][n] = t[j]; }
};

}  // namespace
