// The unaligned-query file's text made on the GPU from the batch and the result streams where an align call left them (included once, by
// xm_capi.hip, behind xm_sam.h, xm_summary.h and xm_result_stage.h): the kernels over the plain rules of xm_unaligned_rules.h.  Four stages, separate launches,
// no launch reads what another workgroup of the same launch wrote:
//   measure   a lane per query walks the query's slice with the summary's walk (xm_summary_rules.h): unalignedFlag[q], and bytes[q] - the closed form of
//             the record's size, 0 for an aligned query; the mates of the unaligned queries are summed over the wavefront and added by its lane 0 to a
//             64-bit counter; a malformed slice leaves the lowest such query in the control word, a record beyond an int32 the lowest such query in another
//   offsets   exclusive sums of the two int32 arrays in query order and both totals: the scan of xm_scan.h
//   compact   a lane per query: an unaligned one stores its index at list[uoff[q]] - the ascending list, so that no wavefront is spent on an aligned query
//   write     a wavefront per list entry composes the record in LDS through xm_sam.h's SamTileSink - names, bases and qualities enter the tile 64 bytes a
//             round, a byte a lane, the bases through the 16-entry table; a tile leaves for HBM as 16-byte pieces with single bytes only in front of the
//             first and behind the last whole piece of the query's range.  No lane stores outside [off[q], off[q + 1]), and no lane loads outside of
//             the batch's arrays, whatever the offsets say (UnalignedTextAt, UnalignedBasesAt).
#pragma once
#include "xm_unaligned_rules.h"
#include <hip/hip_runtime.h>

namespace {

// ctl[0]: the lowest query with a malformed slice, ctl[2]: the lowest query whose record does not fit an int32 (xm::XM_NO_QUERY: none);
// ctl[1]: mates of the unaligned queries; ctl[3]: records that did not end where they were measured to (an internal error)
constexpr int XM_UNALIGNED_CTL_WORDS = 4;

__global__ void __launch_bounds__(256) xm_unaligned_measure_kernel(xm::UnalignedBatch b, xm::ResultStreams st, int32_t* bytes, int32_t* unalignedFlag, unsigned long long* ctl) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long mates = 0;
  if (q < b.nq) {  // (lanes behind the last query stay for the shuffles and add nothing)
    xm::QuerySummary s;
    xm::SummaryNoPenalties none;
    const bool ok = xm::summaryWalkQuery(st, q, s, none);
    if (!ok) atomicMin(&ctl[0], (unsigned long long)q);
    bool unaligned = ok && !s.aligned;
    long long n = unaligned ? xm::unalignedRecordBytes(b, q) : 0;
    if (n > 0x7FFFFFFFll) { atomicMin(&ctl[2], (unsigned long long)q); n = 0; unaligned = false; }
    bytes[q] = (int32_t)n;
    unalignedFlag[q] = unaligned ? 1 : 0;
    if (unaligned) mates = xm::unalignedMates(b, q);
  }
  mates = summaryWaveSum(mates);
  if ((threadIdx.x & 63) == 0 && mates) atomicAdd(&ctl[1], (unsigned long long)mates);
}

__global__ void __launch_bounds__(256) xm_unaligned_compact_kernel(long long nq, const int64_t* uoff, int64_t* list, long long listCap) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const long long u = uoff[q];
  if (uoff[q + 1] > u && u >= 0 && u < listCap) list[u] = q;
}

__global__ void __launch_bounds__(64) xm_unaligned_write_kernel(xm::UnalignedBatch b, const int64_t* list, long long listLength, const int64_t* off, char* text, long long textBytes,
                                                                unsigned long long* ctl) {
  __shared__ __attribute__((aligned(16))) char tile[XM_SAM_TILE_BYTES + xm::XM_SAM_ROOM];
  static_assert(xm::XM_UNALIGNED_ROOM <= xm::XM_SAM_ROOM, "a compose of the unaligned rules fits the tile's room");
  SamTileSink sink;
  sink.tile = tile; sink.out = text; sink.lane = (int)threadIdx.x;
  for (long long i = blockIdx.x; i < listLength; i += gridDim.x) {
    const long long q = list[i];
    if (q < 0 || q >= b.nq) continue;  // (the whole wavefront goes on)
    const long long start = off[q], end = off[q + 1];
    if (start < 0 || start >= end || end > textBytes) continue;
    sink.begin(start, end);
    (void)xm::unalignedWriteQuery(b, q, sink);
    const bool ended = sink.finish();
    if (!ended && threadIdx.x == 0) atomicAdd(&ctl[3], 1ull);
  }
}

}  // namespace
