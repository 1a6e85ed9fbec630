// The text of the pile-up's insertion events, kept on the device while the batch is resident (included once, by xm_capi_pileup.h): the kernels
// over the plain rules of xm_pileup_text_rules.h.  Three stages, separate launches on the context's stream, no launch reads what another workgroup of the
// same launch wrote:
//   measure   a lane per event of the call, in the order the atomic counter appended them: the bytes of text the event keeps (0 for a deletion)
//   offsets   the exclusive sums of those lengths and their total (the scan of xm_scan.h over one 64-bit array)
//   gather    a lane per byte of the text: it finds its event by a binary search over the offsets and writes one letter.  Insertions are a few bases each
//             and a rare one is a thousand: a lane per byte keeps the stores of a wavefront side by side and the long event costs no lane more than a
//             short one, for log2(events) reads of offsets that sit in the cache.  A lane stores byte b only, and only with off[e] <= b < off[e + 1].
#pragma once
#include "xm_pileup_text_rules.h"
#include <hip/hip_runtime.h>

namespace {

// what the stages read: the n events of the call where the pile-up kernel appended them, and the batch they came from (event[4] - queryBase is the query)
struct PileupTextJob {
  const long long* events;
  long long n, queryBase;
  long long nq;
  const int64_t* mateOffset; const int32_t* mateLength; const uint8_t* codes;
};

// the mate an event speaks of and its length; an event whose query is not of this batch has a mate of no bases
__device__ __forceinline__ const uint8_t* ptextMate(const PileupTextJob& j, const long long* ev, int& readLen) {
  const long long q = ev[4] - j.queryBase;
  readLen = 0;
  if (q < 0 || q >= j.nq) return j.codes;
  const int mate = xm::pileupEventMate(ev[5]);
  readLen = j.mateLength[q * 2 + mate];
  return j.codes + j.mateOffset[q * 2 + mate];
}

__global__ void __launch_bounds__(256) xm_ptext_measure_kernel(PileupTextJob j, long long* len) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= j.n) return;
  const long long* ev = j.events + e * xm::XM_PILEUP_EVENT_WORDS;
  int readLen;
  ptextMate(j, ev, readLen);
  len[e] = xm::pileupTextKept(ev[2], ev[3], ev[6], readLen);
}

// textCap: the bytes the text buffer holds (the host sized it for the total; no lane stores behind it whatever the offsets say)
__global__ void __launch_bounds__(256) xm_ptext_gather_kernel(PileupTextJob j, const int64_t* off, char* text, long long textCap) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= off[j.n] || b >= textCap) return;
  long long lo = 0, hi = j.n;  // off[lo] <= b < off[hi]: the event that holds byte b is the last one that starts at or before it (events without text are passed over)
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (off[mid] <= b) lo = mid; else hi = mid;
  }
  const long long* ev = j.events + lo * xm::XM_PILEUP_EVENT_WORDS;
  int readLen;
  const uint8_t* mate = ptextMate(j, ev, readLen);
  const long long i = b - off[lo];
  if (i < 0 || b >= off[lo + 1] || i >= xm::pileupTextKept(ev[2], ev[3], ev[6], readLen)) return;  // (clipped to the event's own range and to its mate)
  text[b] = xm::pileupTextByte(mate, readLen, xm::pileupEventReversed(ev[5]), ev[6], i);
}

// The device side of a pile-up's kept text: lengths, block sums and offsets of the events of a call, and the text, which only grows.
struct PileupTextStage {
  DevBuf<long long> dLen, dBlocks;
  DevBuf<int64_t> dOff;
  DevBuf<char> dText;
  // measure and offsets of the j.n > 0 events, enqueued on s: afterwards dOff[0 .. n] are the offsets and dOff[n] the bytes of the whole text
  void offsets(const PileupTextJob& j, hipStream_t s) {
    dLen.ensure((size_t)j.n); dBlocks.ensure(xmScanSums(j.n, 1)); dOff.ensure((size_t)j.n + 1);
    hipLaunchKernelGGL(xm_ptext_measure_kernel, dim3((unsigned)((j.n + 255) / 256)), dim3(256), 0, s, j, dLen.p);
    xmScan(XmOffsets<long long, 1>{j.n, {dLen.p}, {dOff.p}}, j.n, dBlocks, s);
  }
  // the letters of a text of total > 0 bytes, enqueued on s behind offsets()
  void gather(const PileupTextJob& j, long long total, hipStream_t s) {
    dText.ensure((size_t)total);
    hipLaunchKernelGGL(xm_ptext_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, j, (const int64_t*)dOff.p, dText.p, total);
    HIP_CHECK(hipGetLastError());
  }
};

}  // namespace
