// FASTQ text -> the batch arrays, in HBM (xm_batch_stage_fastq).  The host hands over blocks of whole four-line records as read from the
// file (one text for single reads, two for pairs); the kernels below find the lines, apply the rules of xm_fastq_rules.h to every record, and build
// what xm_batch_stage copies up (mateCount, mateOffset, mateLength, codes, expected, deviation) plus the names and qualities the host's writers read.
// Separate launches, because no launch reads what another workgroup of the same launch wrote (the per-XCD L2s are not coherent):
//   1 line ends   xm_fastq_count_kernel    a tile of XM_FASTQ_TILE_BYTES per block, 16 bytes per lane: the '\n' of the tile are counted
//                 xm_fastq_tiles_kernel    one block: exclusive scan of the tile counts = the line index of each tile's first newline; a text that does
//                                          not end in '\n' gets a virtual line end at `bytes`
//                 xm_fastq_ends_kernel     the tile's lanes again: every newline writes its position to lineEnd[its line index]
//   2 fields      xm_fastq_fields_kernel   a lane per mate slot: the four line bounds of its record -> name, sequence, quality (fastqRecord); the first
//                                          record that is not of the strict form is kept with atomicMin on (file, record)
//                 (with a split size: 2a-2c below - records, the scan of their section counts, a lane per section; stages 3 and 4 then see section slots)
//   3 offsets     the scan of xm_scan.h over FastqMateOffsets
//                                          exclusive sums of the sequence, name and quality lengths in batch order; the host reads the totals to size
//                                          codes, names, quals
//   4 gather      xm_fastq_gather_kernel   a wave per mate, the code table in LDS: bases translated into codes, name and quality bytes copied, 64 bytes a round
// Plain HIP.  Everything is sized by the host from `records` and `bytes`: lineEnd holds 4 * records + 1 entries (FastqText::lineCap), stage 1 writes no entry behind them and
// stage 2 reads none that was not written, whatever the text holds; a text whose line count is not 4 * records is an error the host sees in FastqCtl.
#pragma once
#include "xm_fastq_rules.h"
#include "xm_scan.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace xm {

constexpr int XM_FASTQ_LANE_BYTES = 16;
constexpr int XM_FASTQ_TILE_BYTES = 256 * XM_FASTQ_LANE_BYTES;  // (xm_fastq_tile_bytes(): tests/test_gpu_fastq.py walks the edges this gives)
constexpr unsigned long long XM_FASTQ_NO_ERROR = ~0ull;

// what the host reads back after stage 3
struct FastqCtl {
  unsigned long long firstError;  // XM_FASTQ_NO_ERROR, or (file << 48) | (record << 8) | FastqError of the lowest (file, record) that is not of the strict form
  long long lines[2];             // lines found in each text
  long long totals[3];            // bases, name bytes, quality bytes of the batch
  long long sections;             // the split form: queries of the batch (the sections of all its records), read by the host in front of stage 2c
  long long headers[2];           // FASTA text (xm_fasta.h): the header lines found in each text
};

struct FastqText {
  const char* text;     // allocated up to the next multiple of 16 bytes
  long long bytes, records;
  int32_t* lineEnd;     // [lineCap]
  int32_t* tileCount;   // [tiles] newlines of each tile, then (xm_fastq_tiles_kernel) the line index of its first one
  long long lineCap;    // entries of lineEnd: 4 * records + 1 for FASTQ text; the lines announced + 1 for FASTA text (xm_fasta.h), whose `records` says nothing about its lines
};

// a mate slot's fields as stage 2 leaves them for stages 3 and 4: positions in its file's text
struct FastqMate {
  long long nameAt, seqAt, qualAt;
  int32_t nameLen, seqLen, qualLen, file;
};

// bit 7 of every byte of the word that is '\n' (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t fastqNewlineBits(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(t | x | 0x7F7F7F7Fu);
}

// the lane's 16 bytes of the text as newline bits per word (bytes behind the text never count); -> how many
__device__ __forceinline__ int fastqLaneNewlines(const FastqText& t, long long at, uint32_t bits[4]) {
  bits[0] = bits[1] = bits[2] = bits[3] = 0;
  if (at >= t.bytes) return 0;
  const uint4 v = *reinterpret_cast<const uint4*>(t.text + at);  // (the allocation is padded to 16 bytes)
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const long long valid = t.bytes - at;  // > 0
  int n = 0;
  for (int k = 0; k < 4; k++) {
    uint32_t b = fastqNewlineBits(w[k]);
    const long long left = valid - 4 * k;  // bytes of this word inside the text
    if (left <= 0) b = 0;
    else if (left < 4) b &= (1u << (8 * (int)left)) - 1u;
    bits[k] = b;
    n += __popc(b);
  }
  return n;
}

__global__ void __launch_bounds__(256) xm_fastq_count_kernel(FastqText t) {
  __shared__ int sh[1][256];
  uint32_t bits[4];
  const long long at = (long long)blockIdx.x * XM_FASTQ_TILE_BYTES + (long long)threadIdx.x * XM_FASTQ_LANE_BYTES;
  int count[1] = {fastqLaneNewlines(t, at, bits)};
  xmBlockSum(count, sh);
  if (threadIdx.x == 0) t.tileCount[blockIdx.x] = count[0];
}

// one block: tileCount[] becomes its exclusive scan; lines found (with the virtual one) -> ctl->lines[file]
__global__ void __launch_bounds__(256) xm_fastq_tiles_kernel(FastqText t, long long nTiles, int file, FastqCtl* ctl) {
  __shared__ long long sh[1][256];
  const long long per = (nTiles + 255) / 256;
  const long long a = (long long)threadIdx.x * per, b = a + per < nTiles ? a + per : nTiles;
  long long mine = 0;
  for (long long i = a; i < b; i++) mine += t.tileCount[i];
  long long upTo[1] = {mine};
  xmBlockScan(upTo, sh);
  long long run = upTo[0] - mine;
  for (long long i = a; i < b; i++) { const int c = t.tileCount[i]; t.tileCount[i] = (int32_t)run; run += c; }  // (a text holds less than 2^31 bytes)
  if (threadIdx.x == 0) {
    long long lines = sh[0][255];
    if (t.bytes > 0 && t.text[t.bytes - 1] != '\n') {  // the last block of a file may lack the final newline
      if (lines < t.lineCap) t.lineEnd[lines] = (int32_t)t.bytes;
      lines++;
    }
    ctl->lines[file] = lines;
  }
}

__global__ void __launch_bounds__(256) xm_fastq_ends_kernel(FastqText t) {
  __shared__ int sh[1][256];
  uint32_t bits[4];
  const long long at = (long long)blockIdx.x * XM_FASTQ_TILE_BYTES + (long long)threadIdx.x * XM_FASTQ_LANE_BYTES;
  const int mine = fastqLaneNewlines(t, at, bits);
  int upTo[1] = {mine};
  xmBlockScan(upTo, sh);
  long long line = (long long)t.tileCount[blockIdx.x] + upTo[0] - mine;
  const long long cap = t.lineCap;
  for (int k = 0; k < 4; k++) {
    uint32_t b = bits[k];
    while (b) {
      const int byte = (__ffs((int)b) - 1) >> 3;
      b &= b - 1;
      if (line < cap) t.lineEnd[line] = (int32_t)(at + 4 * k + byte);
      line++;
    }
  }
}

// What stage 2 writes: the fields of every mate slot, and of the batch arrays what needs no offsets.
struct FastqFieldsOut {
  FastqMate* mates;        // [2 nq]
  int32_t* mateCount;      // [nq]
  int32_t* mateLength;     // [2 nq]
  double* expected;        // [nq]
  double* deviation;       // [nq]
  uint8_t* hasQual;        // [2 nq]
  FastqCtl* ctl;
};

__global__ void __launch_bounds__(256) xm_fastq_fields_kernel(FastqText t0, FastqText t1, long long nq, int paired, double expectedInner, double deviation, FastqFieldsOut out) {
  const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= 2 * nq) return;
  const long long q = slot >> 1;
  const int file = paired ? (int)(slot & 1) : 0;
  FastqMate m;
  m.nameAt = m.seqAt = m.qualAt = 0;
  m.nameLen = m.seqLen = m.qualLen = 0;
  m.file = file;
  const bool padding = fastqPaddingMate(slot, paired != 0);
  if ((slot & 1) == 0) {
    out.mateCount[q] = paired ? 2 : 1;
    out.expected[q] = paired ? expectedInner : 0.0;  // (a single query: expected inner distance 0, deviation 1, as hostio.Batch gives them)
    out.deviation[q] = paired ? deviation : 1.0;
  }
  const FastqText& t = file ? t1 : t0;
  // a text that does not hold four lines per record (the host sees it in ctl->lines and stages nothing): the records whose four line ends were found and
  // kept are still looked at, so that an empty line between two records is named where it stands
  const long long l = 4 * q;
  const long long found = out.ctl->lines[file], kept = 4 * t.records + 1;
  if (!padding && l + 3 < (found < kept ? found : kept)) {
    const long long s0 = l == 0 ? 0 : (long long)t.lineEnd[l - 1] + 1;
    const long long e0 = t.lineEnd[l], e1 = t.lineEnd[l + 1], e2 = t.lineEnd[l + 2], e3 = t.lineEnd[l + 3];
    FastqFields f;
    const int err = fastqRecord(t.text, s0, e0, e0 + 1, e1, e2 + 1, e3, f);
    if (err != XM_FQ_OK) atomicMin(&out.ctl->firstError, ((unsigned long long)file << 48) | ((unsigned long long)q << 8) | (unsigned long long)err);
    else {
      m.nameAt = f.nameAt; m.seqAt = f.seqAt; m.qualAt = f.qualAt;
      m.nameLen = (int32_t)f.nameLen; m.seqLen = (int32_t)f.seqLen; m.qualLen = (int32_t)f.qualLen;
    }
  }
  out.mates[slot] = m;
  out.mateLength[slot] = m.seqLen;
  out.hasQual[slot] = padding ? 0 : 1;
}

// ---- the split form of stage 2 (split_past_size > 0, single reads): a record becomes its SequenceSplitter sections, each a query.  Three steps
// in the place of xm_fastq_fields_kernel, each its own launch(es); the host reads the query count between the second and the third to size the slot arrays.
//   2a records    xm_fastq_split_records_kernel   a lane per record: fastqRecordSplit -> the record's fields and how many sections it gives
//   2b first      the scan of xm_scan.h over FastqSplitFirst
//                                                 exclusive sums of the section counts: first[r] = the first query of record r, first[records] = ctl->sections
//   2c sections   xm_fastq_split_sections_kernel  a lane per query: its record by binary search over first[], its section by fastqSectionMate -> both mate slots
__global__ void __launch_bounds__(256) xm_fastq_split_records_kernel(FastqText t, long long split, FastqMate* recs, int32_t* counts, FastqCtl* ctl) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= t.records) return;
  FastqMate m;
  m.nameAt = m.seqAt = m.qualAt = 0;
  m.nameLen = m.seqLen = m.qualLen = 0;
  m.file = 0;
  int32_t count = 0;
  const long long l = 4 * r;
  const long long found = ctl->lines[0], kept = 4 * t.records + 1;  // (as xm_fastq_fields_kernel: only records whose four line ends were found and kept)
  if (l + 3 < (found < kept ? found : kept)) {
    const long long s0 = l == 0 ? 0 : (long long)t.lineEnd[l - 1] + 1;
    const long long e0 = t.lineEnd[l], e1 = t.lineEnd[l + 1], e2 = t.lineEnd[l + 2], e3 = t.lineEnd[l + 3];
    FastqFields f;
    const int err = fastqRecordSplit(t.text, s0, e0, e0 + 1, e1, e2 + 1, e3, f);
    if (err != XM_FQ_OK) atomicMin(&ctl->firstError, ((unsigned long long)r << 8) | (unsigned long long)err);
    else {
      m.nameAt = f.nameAt; m.seqAt = f.seqAt;
      m.nameLen = (int32_t)f.nameLen; m.seqLen = (int32_t)f.seqLen;  // (a text holds at most 2^30 bytes)
      count = (int32_t)fastqSectionCount(f.seqLen, split);
    }
  }
  recs[r] = m;
  counts[r] = count;
}

// stage 2b's Items (xm_scan.h): first[r] = the sections in front of record r, first[records] = ctl->sections = all of them
struct FastqSplitFirst {
  static constexpr int N = 1;
  long long records;
  const int32_t* counts;
  int64_t* first; FastqCtl* ctl;
  __device__ long long count() const { return records; }
  __device__ void lens(long long r, long long v[1]) const { v[0] = counts[r]; }
  __device__ void put(long long r, const long long at[1]) const { first[r] = at[0]; }
  __device__ void totals(const long long t[1]) const { first[records] = t[0]; ctl->sections = t[0]; }
};

// nq = first[records] as the host read it, which sized out's arrays: no lane writes behind them
__global__ void __launch_bounds__(256) xm_fastq_split_sections_kernel(long long nq, long long records, const FastqMate* recs, const int64_t* first, FastqFieldsOut out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq || records < 1 || first[records] != nq) return;
  long long lo = 0, hi = records;  // first[lo] <= q < first[hi]: the last record that starts at or in front of q is the one that holds it (its count is > 0)
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (first[mid] <= q) lo = mid; else hi = mid;
  }
  const FastqMate rec = recs[lo];
  FastqFields rf, sf;
  rf.nameAt = rec.nameAt; rf.seqAt = rec.seqAt; rf.qualAt = rec.qualAt;
  rf.nameLen = rec.nameLen; rf.seqLen = rec.seqLen; rf.qualLen = rec.qualLen;
  fastqSectionMate(rf, first[lo + 1] - first[lo], q - first[lo], sf);
  FastqMate m;
  m.nameAt = sf.nameAt; m.seqAt = sf.seqAt; m.qualAt = sf.qualAt;
  m.nameLen = (int32_t)sf.nameLen; m.seqLen = (int32_t)sf.seqLen; m.qualLen = 0;
  m.file = 0;
  FastqMate pad;
  pad.nameAt = pad.seqAt = pad.qualAt = 0;
  pad.nameLen = pad.seqLen = pad.qualLen = 0;
  pad.file = 0;
  out.mates[2 * q] = m;
  out.mates[2 * q + 1] = pad;
  out.mateCount[q] = 1;
  out.expected[q] = 0.0;
  out.deviation[q] = 1.0;
  out.mateLength[2 * q] = m.seqLen;
  out.mateLength[2 * q + 1] = 0;
  out.hasQual[2 * q] = 0;
  out.hasQual[2 * q + 1] = 0;
}

// ---- stage 3: the scan (xm_scan.h) of the sequence, name and quality lengths of the mate slots; without qualities the third is 0 and qualOff is null
struct FastqMateOffsets {
  static constexpr int N = 3;
  long long slots;
  const FastqMate* mates; int keepQual;
  int64_t* mateOffset; int64_t* nameOff; int64_t* qualOff; FastqCtl* ctl;
  __device__ long long count() const { return slots; }
  __device__ void lens(long long i, long long v[3]) const { const FastqMate& m = mates[i]; v[0] = m.seqLen; v[1] = m.nameLen; v[2] = keepQual ? m.qualLen : 0; }
  __device__ void put(long long i, const long long off[3]) const {
    mateOffset[i] = mates[i].seqLen > 0 ? off[0] : 0;  // (the padding mate of a single query: offset 0)
    nameOff[i] = off[1];
    if (qualOff) qualOff[i] = off[2];
  }
  __device__ void totals(const long long t[3]) const {
    for (int j = 0; j < 3; j++) ctl->totals[j] = t[j];
    nameOff[slots] = t[1];
    if (qualOff) qualOff[slots] = t[2];
  }
};

// ---- stage 4: a wave per mate slot, four to a block
__global__ void __launch_bounds__(256) xm_fastq_gather_kernel(long long slots, const FastqMate* mates, const char* text0, const char* text1, const int64_t* mateOffset, const int64_t* nameOff,
                                                              const int64_t* qualOff, uint8_t* codes, char* names, char* quals) {
  __shared__ uint8_t table[256];
  table[threadIdx.x] = fastqCode((unsigned char)threadIdx.x);
  __syncthreads();
  const long long slot = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63u);
  if (slot >= slots) return;
  const FastqMate m = mates[slot];
  const char* text = m.file ? text1 : text0;
  if (m.seqLen > 0) {
    const unsigned char* src = (const unsigned char*)text + m.seqAt;
    uint8_t* dst = codes + mateOffset[slot];
    for (int i = lane; i < m.seqLen; i += 64) dst[i] = table[src[i]];
  }
  if (m.nameLen > 0) {
    const char* src = text + m.nameAt;
    char* dst = names + nameOff[slot];
    for (int i = lane; i < m.nameLen; i += 64) dst[i] = src[i];
  }
  if (quals && m.qualLen > 0) {
    const char* src = text + m.qualAt;
    char* dst = quals + qualOff[slot];
    for (int i = lane; i < m.qualLen; i += 64) dst[i] = src[i];
  }
}

}  // namespace xm
