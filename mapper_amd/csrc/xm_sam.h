// SAM records formatted on the GPU from the result streams where an align call left them (included once, by xm_capi.hip): the kernels over the
// plain rules of xm_sam_rules.h.  Three stages, separate launches, no launch reads what another workgroup of the same launch wrote:
//   measure   a lane per query walks the query's slice with the sink that only counts: bytes and records per query (0 for an unaligned one); a malformed
//             slice leaves the lowest such query in the control words
//   offsets   exclusive sums of the bytes in query order and both totals (the scan of xm_scan.h over SamSums, placed over SamByteOffsets)
//   write     a wavefront per query walks the slice again with the sink that composes the text in LDS, a tile of XM_SAM_TILE_BYTES bytes that lies where the
//             text buffer's own tiles lie: names, contig names and SEQ go into the tile 64 bytes a round (a byte a lane), the short fields are composed there
//             by lane 0, and a tile leaves for HBM as 16-byte pieces, 64 a round, with single bytes only in front of the first and behind the last whole piece
//             of the query's range.  No lane stores outside [offset[q], offset[q + 1]).
#pragma once
#include "xm_sam_rules.h"
#include <hip/hip_runtime.h>

namespace {

constexpr int XM_SAM_TILE_BYTES = 1024;  // one round of 16-byte stores of a wavefront (xm_sam_tile_bytes(): tests put record ends on both sides of the multiples)

// what a format call reads; the control words: [0] the lowest query with a malformed slice (xm::XM_NO_QUERY: none), [1] queries whose text did not end where
// it was measured to (an internal error), [2] bytes of the whole text, [3] its records
struct SamJob {
  xm::SamBatch batch;
  xm::ResultStreams streams;
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

// The offsets stage's two Items (xm_scan.h): the sums pass takes bytes and records per query and leaves the totals; the place pass needs the offsets of the
// bytes only, so it runs over that one array (the records are not read a second time).
struct SamSums {
  static constexpr int N = 2;
  long long nq;
  const long long* bytes; const long long* records;
  long long* offset; unsigned long long* ctl;
  __device__ long long count() const { return nq; }
  __device__ void lens(long long q, long long v[2]) const { v[0] = bytes[q]; v[1] = records[q]; }
  __device__ void totals(const long long t[2]) const { offset[nq] = t[0]; ctl[2] = (unsigned long long)t[0]; ctl[3] = (unsigned long long)t[1]; }
};
struct SamByteOffsets {
  static constexpr int N = 1;
  long long nq;
  const long long* bytes;
  long long* offset;
  __device__ long long count() const { return nq; }
  __device__ void lens(long long q, long long v[1]) const { v[0] = bytes[q]; }
  __device__ void put(long long q, const long long off[1]) const { offset[q] = off[0]; }
};

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
