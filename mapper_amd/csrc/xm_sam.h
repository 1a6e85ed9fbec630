// SAM records formatted on the GPU from the result streams where an align call left them (included once, by xm_capi.hip): the kernels over the
// plain rules of xm_sam_rules.h.  Three stages, separate launches, no launch reads what another workgroup of the same launch wrote:
//   measure   a lane per query walks the query's slice with the sink that only counts: bytes and records per query (0 for an unaligned one); a malformed
//             slice leaves the lowest such query in the control words
//   offsets   exclusive sums of the bytes in query order and both totals (three kernels, as xm_result_stage.h's scan: 4096 queries a block)
//   write     a wavefront per query walks the slice again with the sink that composes the text in LDS, a tile of XM_SAM_TILE_BYTES bytes that lies where the
//             text buffer's own tiles lie: names, contig names and SEQ go into the tile 64 bytes a round (a byte a lane), the short fields are composed there
//             by lane 0, and a tile leaves for HBM as 16-byte pieces, 64 a round, with single bytes only in front of the first and behind the last whole piece
//             of the query's range.  No lane stores outside [offset[q], offset[q + 1]).
#pragma once
#include "xm_sam_rules.h"
#include <hip/hip_runtime.h>

namespace {

constexpr int XM_SAM_TILE_BYTES = 1024;  // one round of 16-byte stores of a wavefront (xm_sam_tile_bytes(): tests put record ends on both sides of the multiples)
constexpr int XM_SAM_SCAN_PER_THREAD = 16;
constexpr int XM_SAM_SCAN_PER_BLOCK = 256 * XM_SAM_SCAN_PER_THREAD;
constexpr unsigned long long XM_SAM_NO_ERROR = ~0ull;

// what a format call reads; the control words: [0] the lowest query with a malformed slice (XM_SAM_NO_ERROR: none), [1] queries whose text did not end where
// it was measured to (an internal error), [2] bytes of the whole text, [3] its records
struct SamJob {
  xm::SamBatch batch;
  xm::SamStreams streams;
  xm::SamContigs contigs;
};

__global__ void __launch_bounds__(256) xm_sam_measure_kernel(SamJob j, long long* bytes, long long* records, unsigned long long* ctl) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= j.batch.nq) return;
  xm::SamCount count;
  if (!xm::samWalkQuery(j.batch, j.streams, j.contigs, q, count)) {
    atomicMin(&ctl[0], (unsigned long long)q);
    count.bytes = 0; count.records = 0;
  }
  bytes[q] = count.bytes; records[q] = count.records;
}

__global__ void __launch_bounds__(256) xm_sam_totals_kernel(long long nq, const long long* bytes, const long long* records, long long* blockSums) {
  __shared__ long long shA[256], shB[256];
  const long long base = (long long)blockIdx.x * XM_SAM_SCAN_PER_BLOCK + (long long)threadIdx.x * XM_SAM_SCAN_PER_THREAD;
  long long a = 0, b = 0;
  for (int k = 0; k < XM_SAM_SCAN_PER_THREAD; k++) if (base + k < nq) { a += bytes[base + k]; b += records[base + k]; }
  shA[threadIdx.x] = a; shB[threadIdx.x] = b;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) { shA[threadIdx.x] += shA[threadIdx.x + d]; shB[threadIdx.x] += shB[threadIdx.x + d]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { blockSums[2 * blockIdx.x] = shA[0]; blockSums[2 * blockIdx.x + 1] = shB[0]; }
}

__global__ void xm_sam_blocks_kernel(long long nBlocks, long long nq, long long* blockSums, long long* offset, unsigned long long* ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long a = 0, b = 0;
  for (long long i = 0; i < nBlocks; i++) { const long long x = blockSums[2 * i], y = blockSums[2 * i + 1]; blockSums[2 * i] = a; blockSums[2 * i + 1] = b; a += x; b += y; }
  offset[nq] = a;
  ctl[2] = (unsigned long long)a; ctl[3] = (unsigned long long)b;
}

__global__ void __launch_bounds__(256) xm_sam_offsets_kernel(long long nq, const long long* bytes, const long long* blockSums, long long* offset) {
  __shared__ long long sh[256];
  const long long base = (long long)blockIdx.x * XM_SAM_SCAN_PER_BLOCK + (long long)threadIdx.x * XM_SAM_SCAN_PER_THREAD;
  long long a = 0;
  for (int k = 0; k < XM_SAM_SCAN_PER_THREAD; k++) if (base + k < nq) a += bytes[base + k];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele scan of the 256 thread totals
    long long x = 0;
    if ((int)threadIdx.x >= d) x = sh[threadIdx.x - d];
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  long long off = blockSums[2 * blockIdx.x] + sh[threadIdx.x] - a;
  for (int k = 0; k < XM_SAM_SCAN_PER_THREAD; k++) if (base + k < nq) { offset[base + k] = off; off += bytes[base + k]; }
}

// The sink of the write kernel: one wavefront (a workgroup of 64 lanes, so __syncthreads() is the wavefront's barrier), every call made by all of its lanes
// with the same arguments.  tile[0] is byte `base` of the text, base a multiple of XM_SAM_TILE_BYTES; tile[lo, fill) is text of this query that has not left yet.
struct SamTileSink {
  char* tile;       // LDS, XM_SAM_TILE_BYTES + XM_SAM_ROOM bytes, 16-byte aligned (a compose may run over the tile's end by less than XM_SAM_ROOM)
  char* out;        // the text buffer, 16-byte aligned
  long long base, end;
  int lo, fill, lane;

  __device__ void begin(long long start, long long end_) {
    base = start & ~(long long)(XM_SAM_TILE_BYTES - 1);
    lo = fill = (int)(start - base);
    end = end_;
  }
  // tile[lo, hi) to the text (never behind the query's end, whatever the walk produced)
  __device__ void store(int hi) {
    __syncthreads();
    if ((long long)hi > end - base) hi = (int)(end - base);
    if (hi > lo) {
      const int firstWhole = (lo + 15) & ~15;
      const int a = firstWhole < hi ? firstWhole : hi;  // [lo, a) single bytes, [a, b) 16-byte pieces, [b, hi) single bytes
      const int b = (hi & ~15) > a ? (hi & ~15) : a;
      char* dst = out + base;
      if (lane < a - lo) dst[lo + lane] = tile[lo + lane];
      for (int p = a + 16 * lane; p < b; p += 16 * 64) *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(tile + p);
      if (lane < hi - b) dst[b + lane] = tile[b + lane];
    }
    __syncthreads();
  }
  // a full tile leaves; what ran over its end becomes the start of the next one
  __device__ void turn() {
    store(XM_SAM_TILE_BYTES);
    const int over = fill - XM_SAM_TILE_BYTES;
    char c = 0;
    if (lane < over) c = tile[XM_SAM_TILE_BYTES + lane];
    __syncthreads();
    if (lane < over) tile[lane] = c;
    base += XM_SAM_TILE_BYTES;
    fill = over; lo = 0;
  }
  template <class F>
  __device__ void compose(F f) {
    int n = 0;
    if (lane == 0) n = f(tile + fill);
    n = __shfl(n, 0);
    fill += n;
    if (fill >= XM_SAM_TILE_BYTES) turn();
  }
  // n bytes, byte i = byteAt(i), 64 a round
  template <class G>
  __device__ void spread(long long n, G byteAt) {
    long long done = 0;
    while (done < n) {
      const long long room = XM_SAM_TILE_BYTES - fill;
      const int c = (int)(n - done < room ? n - done : room);
      for (int i = lane; i < c; i += 64) tile[fill + i] = byteAt(done + i);
      fill += c; done += c;
      if (fill >= XM_SAM_TILE_BYTES) turn();
    }
  }
  __device__ void bytesAt(const char* p, long long n) { spread(n, [=](long long i) { return p[i]; }); }
  __device__ void seq(const uint8_t* codes, int n, bool rev) { spread(n, [=](long long i) { return xm::samSeqBase(codes, n, rev, (int)i); }); }
  __device__ void endRecord() {}
  // the rest leaves; true: the text ended where it was measured to
  __device__ bool finish() {
    const bool ok = base + fill == end;
    store(fill);
    return ok;
  }
};

__global__ void __launch_bounds__(64) xm_sam_write_kernel(SamJob j, const long long* offset, char* text, unsigned long long* ctl) {
  __shared__ __attribute__((aligned(16))) char tile[XM_SAM_TILE_BYTES + xm::XM_SAM_ROOM];
  SamTileSink sink;
  sink.tile = tile; sink.out = text; sink.lane = (int)threadIdx.x;
  for (long long q = blockIdx.x; q < j.batch.nq; q += gridDim.x) {
    const long long start = offset[q], end = offset[q + 1];
    if (start >= end) continue;  // (an unaligned query: the whole wavefront goes on)
    sink.begin(start, end);
    const bool walked = xm::samWalkQuery(j.batch, j.streams, j.contigs, q, sink);
    const bool ended = sink.finish();
    if ((!walked || !ended) && threadIdx.x == 0) atomicAdd(&ctl[1], 1ull);
  }
}

// Test hook (xm_test_format_doubles): Double.toString of n values, a lane each, 24 bytes a value
__global__ void __launch_bounds__(256) xm_sam_doubles_kernel(long long n, const double* x, char* out24, int32_t* len) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  char s[xm::XM_SAM_DOUBLE_BYTES];
  const int m = xm::samPutDouble(s, x[i]);
  for (int k = 0; k < xm::XM_SAM_DOUBLE_BYTES; k++) out24[i * xm::XM_SAM_DOUBLE_BYTES + k] = k < m ? s[k] : 0;
  len[i] = m;
}

}  // namespace
