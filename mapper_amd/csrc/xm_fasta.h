// FASTA text -> the batch arrays, in HBM (xm_batch_stage_fasta).  What xm_fastq.h does for four-line FASTQ records, for '>' records of any
// number of lines: the bases of a record are not one slice of the text but the trimmed body lines one behind the other, so mates, sections and the gather
// work on base ordinals (xm_fasta_rules.h), and baseBefore[] is the map from ordinals back to the text.  Separate launches, because no launch reads what
// another workgroup of the same launch wrote (the per-XCD L2s are not coherent):
//   1 line ends   xm_fastq_count / tiles / ends_kernel (xm_fastq.h, unchanged), with FastqText::lineCap = the lines announced + 1
//   2 lines       xm_fasta_lines_kernel          a lane per line: header or body, where its name or its trimmed bases start, how many bases it adds
//   3 line scans  the scan of xm_scan.h over FastaLineOffsets
//                                                exclusive sums of the header flags and of the trimmed lengths: header r
//                                                scatters recLine[r], every line gets baseBefore[line]; recLine[records] = lines, baseBefore[lines] = the bases;
//                                                the headers found go to FastqCtl::headers for the host's check of the strict form
//   4 records     xm_fasta_records_kernel        a lane per mate slot: the name from the header line, first = baseBefore[recLine[r]], length from recLine[r + 1]
//                 (with a split size: xm_fasta_split_records_kernel, a lane per record, then stages 2b and 2c of xm_fastq.h as they are)
//   5 offsets     stage 3 of xm_fastq.h as it is (it reads lengths only)
//   6 gather      xm_fasta_gather_kernel         a wave per mate slot: a window of 64 lines held one per lane, 64 consecutive bases a round, each lane finding
//                                                its line in the window in six steps
// Everything is sized by the host from `bytes`, `records` and `lines`; a text whose headers or lines are not the ones announced is an error the host sees in
// FastqCtl, and until then every kernel reads only the lines that were found and kept (fastaLinesKept) and writes inside what the announced counts sized.
#pragma once
#include "xm_fasta_rules.h"
#include "xm_fastq.h"

namespace xm {

// the per-line arrays of one text (about 16 bytes a line with lineEnd) and its records' header lines
struct FastaLines {
  long long lines;       // announced: lineStart, lineBases, lineHeader hold `lines` entries, baseBefore lines + 1, recLine records + 1
  int32_t* lineStart;    // header: the position of its '>'; body: where its trimmed bases start
  int32_t* lineBases;    // the bases the line adds (0 for a header)
  uint8_t* lineHeader;
  int32_t* baseBefore;   // a text holds at most 2^30 bytes: int32 suffices
  int32_t* recLine;
};

// the lines stages 2 to 6 look at: those found (FastqCtl::lines, a launch earlier) and kept (no more than announced)
__device__ __forceinline__ long long fastaLinesKept(const FastqCtl* ctl, int file, const FastaLines& L) {
  const long long found = ctl->lines[file];
  return found < L.lines ? found : L.lines;
}
// the text holds what was announced: only then recLine[] is complete
__device__ __forceinline__ bool fastaCountsHold(const FastqCtl* ctl, int file, const FastqText& t, const FastaLines& L) {
  return ctl->lines[file] == L.lines && ctl->headers[file] == t.records;
}
__device__ __forceinline__ unsigned long long fastaErrorKey(int file, long long record, int err) {
  return ((unsigned long long)file << 48) | ((unsigned long long)record << 8) | (unsigned long long)err;
}

__global__ void __launch_bounds__(256) xm_fasta_lines_kernel(FastqText t, FastaLines L, int file, FastqCtl* ctl) {
  const long long line = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (line == 0 && t.text[0] != '>') atomicMin(&ctl->firstError, fastaErrorKey(file, 0, XM_FA_NO_HEADER));
  if (line >= fastaLinesKept(ctl, file, L)) return;
  const long long start = line == 0 ? 0 : (long long)t.lineEnd[line - 1] + 1;
  long long at, length;
  const bool header = fastaLine(t.text, start, t.lineEnd[line], at, length);
  L.lineStart[line] = (int32_t)(header ? start : at);
  L.lineBases[line] = header ? 0 : (int32_t)length;
  L.lineHeader[line] = header ? 1 : 0;
}

// stage 3's Items (xm_scan.h) over the lines kept: (header flag, bases) per line
struct FastaLineOffsets {
  static constexpr int N = 2;
  FastaLines L;
  long long records;  // announced: recLine holds records + 1 entries
  int file;
  FastqCtl* ctl;
  __device__ long long count() const { return fastaLinesKept(ctl, file, L); }
  __device__ void lens(long long line, long long v[2]) const { v[0] = L.lineHeader[line]; v[1] = L.lineBases[line]; }
  __device__ void put(long long line, const long long off[2]) const {
    L.baseBefore[line] = (int32_t)off[1];
    if (L.lineHeader[line] && off[0] < records) L.recLine[off[0]] = (int32_t)line;  // (more headers than announced: the host sees it in FastqCtl::headers)
  }
  __device__ void totals(const long long t[2]) const {
    const long long n = count();
    ctl->headers[file] = t[0];
    L.baseBefore[n] = (int32_t)t[1];
    L.recLine[records] = (int32_t)n;
  }
};

// record r of a text whose counts hold -> its name and its ordinals; false: nothing to read (the host refuses the text by its counts)
__device__ __forceinline__ bool fastaRecordOf(const FastqText& t, const FastaLines& L, int file, const FastqCtl* ctl, long long r, FastqMate& m) {
  m.nameAt = m.seqAt = m.qualAt = 0;
  m.nameLen = m.seqLen = m.qualLen = 0;
  m.file = file | XM_FASTA_ORDINAL;
  if (!fastaCountsHold(ctl, file, t, L) || r >= t.records) return false;
  const long long line = L.recLine[r], next = L.recLine[r + 1];
  long long at, length;
  fastaLine(t.text, L.lineStart[line], t.lineEnd[line], at, length);  // (a header: the name)
  m.nameAt = at;
  m.nameLen = (int32_t)length;
  m.seqAt = L.baseBefore[line];
  m.seqLen = (int32_t)((long long)L.baseBefore[next] - m.seqAt);
  return true;
}

__global__ void __launch_bounds__(256) xm_fasta_records_kernel(FastqText t0, FastqText t1, FastaLines L0, FastaLines L1, long long nq, int paired, double expectedInner, double deviation,
                                                               FastqFieldsOut out) {
  const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= 2 * nq) return;
  const long long q = slot >> 1;
  const int file = paired ? (int)(slot & 1) : 0;
  if ((slot & 1) == 0) {
    out.mateCount[q] = paired ? 2 : 1;
    out.expected[q] = paired ? expectedInner : 0.0;
    out.deviation[q] = paired ? deviation : 1.0;
  }
  FastqMate m;
  m.nameAt = m.seqAt = m.qualAt = 0;
  m.nameLen = m.seqLen = m.qualLen = 0;
  m.file = file | XM_FASTA_ORDINAL;
  if (!fastqPaddingMate(slot, paired != 0) && fastaRecordOf(file ? t1 : t0, file ? L1 : L0, file, out.ctl, q, m)) {
    const int err = fastaRecordError(m.seqLen, 0);
    if (err != XM_FA_OK) {
      atomicMin(&out.ctl->firstError, fastaErrorKey(file, q, err));
      m.seqLen = m.nameLen = 0;  // (nothing is staged; the offsets stay inside what the text could give)
    }
  }
  out.mates[slot] = m;
  out.mateLength[slot] = m.seqLen;
  out.hasQual[slot] = 0;  // a FASTA mate has no quality
}

// stage 2a of the split form for FASTA text: a lane per record -> its fields (seqAt an ordinal: fastqSectionMate works on it as it stands) and its section count
__global__ void __launch_bounds__(256) xm_fasta_split_records_kernel(FastqText t, FastaLines L, long long split, FastqMate* recs, int32_t* counts, FastqCtl* ctl) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= t.records) return;
  FastqMate m;
  int32_t count = 0;
  if (fastaRecordOf(t, L, 0, ctl, r, m)) {
    const int err = fastaRecordError(m.seqLen, split);
    if (err != XM_FA_OK) atomicMin(&ctl->firstError, fastaErrorKey(0, r, err));
    else count = (int32_t)fastqSectionCount(m.seqLen, split);
  }
  recs[r] = m;
  counts[r] = count;
}

// ---- stage 6: a wave per mate slot, four to a block.  The mate is the ordinals [b0, b0 + seqLen) of its file.  The wave holds a window of 64 lines, lane k
// the baseBefore and the start of line first + k; a round takes 64 consecutive ordinals, and each lane finds its line by six steps of a search over the window
// (the entries come from the other lanes through the LDS crossbar: __shfl, no LDS memory and no barrier), so lane use does not depend on the column width.
struct FastaGatherText {
  const char* text;
  long long bytes;
  const int32_t* lineStart;
  const int32_t* baseBefore;
  long long lines;  // announced; the host launches this stage only for texts whose counts hold
};

__global__ void __launch_bounds__(256) xm_fasta_gather_kernel(long long slots, const FastqMate* mates, FastaGatherText g0, FastaGatherText g1, const int64_t* mateOffset, const int64_t* nameOff,
                                                              uint8_t* codes, char* names) {
  __shared__ uint8_t table[256];
  table[threadIdx.x] = fastqCode((unsigned char)threadIdx.x);
  __syncthreads();
  const long long slot = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63u);
  if (slot >= slots) return;
  const FastqMate m = mates[slot];
  const FastaGatherText& g = (m.file & 1) ? g1 : g0;
  if (m.seqLen > 0) {
    uint8_t* dst = codes + mateOffset[slot];
    const long long b0 = m.seqAt, b1 = m.seqAt + m.seqLen;
    long long first = fastaLineOf(g.baseBefore, g.lines, b0);  // (the same search in every lane)
    long long at = b0;
    while (at < b1 && first < g.lines) {
      const long long mine = first + lane < g.lines ? first + lane : g.lines;  // lines behind the text: no bases, they start at the text's last ordinal + 1
      const int bb = g.baseBefore[mine];
      const int st = mine < g.lines ? g.lineStart[mine] : 0;
      const long long last = first + 64 < g.lines ? first + 64 : g.lines;
      const long long windowEnd = g.baseBefore[last];  // the ordinals of the window: [baseBefore[first], windowEnd)
      const long long stop = windowEnd < b1 ? windowEnd : b1;
      for (long long round = at; round < stop; round += 64) {  // (every lane stays in the loop: a lane that left it would hand nothing to __shfl)
        const long long o = round + lane < stop ? round + lane : stop - 1;
        int k = 0;  // the last k of the window with baseBefore <= o (entry 0 qualifies: baseBefore[first] <= at)
        for (int step = 32; step > 0; step >>= 1) {
          const int probe = __shfl(bb, k + step, 64);
          if ((long long)probe <= o) k += step;
        }
        const long long src = (long long)__shfl(st, k, 64) + (o - (long long)__shfl(bb, k, 64));
        const long long i = o - b0;
        if (round + lane < stop && i >= 0 && i < m.seqLen && src >= 0 && src < g.bytes) dst[i] = table[(unsigned char)g.text[src]];
      }
      at = stop > at ? stop : at;
      first = last;
    }
  }
  if (m.nameLen > 0) {
    const char* src = g.text + m.nameAt;
    char* dst = names + nameOff[slot];
    for (int i = lane; i < m.nameLen; i += 64) dst[i] = src[i];
  }
}

}  // namespace xm
