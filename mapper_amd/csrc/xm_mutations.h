// The end of --out-mutations on the device (included once, by xm_capi.hip): the kernels that move the counts of one pile-up into another
// (absorb), pick the SNP rows out of a pile-up in position-then-letter order (select: count, a scan over the block counts, place) and judge indel candidates
// over the middle depth (judge).  What a row or a verdict is, is xm_mutations_rules.h's to say; nothing here decides.  Every load and store goes through a global
// pointer; nothing is handed from one workgroup to another inside a launch - the launches of a stream follow each other.
#pragma once
#include "xm_mutations_rules.h"
#include <hip/hip_runtime.h>

#define XM_MUTATIONS_THREADS 256
#define XM_MUTATIONS_TILES 4
#define XM_MUTATIONS_BLOCK (XM_MUTATIONS_THREADS * XM_MUTATIONS_TILES)  // forward positions a block of the select kernels takes
#define XM_MUTATIONS_SCAN_BLOCK 1024                                     // entries a block of the scan kernels takes (four a thread)

namespace {

// a SNP row as the kernels write it: xm_snp_row's layout (include/xmapper_hip.h)
struct MutationsSnpRow {
  int32_t contig, position;
  uint8_t letter, referenceCode, reserved[6];
  unsigned long long supportUnits, totalUnits;
};
static_assert(sizeof(MutationsSnpRow) == 32, "xm_snp_row is 32 bytes");

// an indel candidate and its verdict: xm_indel_candidate's and xm_indel_verdict's layouts
struct MutationsCandidate {
  int32_t contig, kind;
  int64_t pos1, length;
  unsigned long long supportUnits;
};
struct MutationsVerdict {
  unsigned long long totalUnits;
  int64_t keep;
};
static_assert(sizeof(MutationsCandidate) == 32 && sizeof(MutationsVerdict) == 16, "the layouts of include/xmapper_hip.h");

// the counts of a pile-up where they lie in HBM (mid null: no query-end fraction, the middle depth is the depth)
struct MutationsCounts {
  unsigned long long* depth;  // [total]
  unsigned long long* alt;    // [4][total]
  unsigned long long* mid;    // [total] or null
  long long total;
};

// ---------------------------------------------------------------- absorb
// into[i] += from[i]; from[i] = 0 over up to three arrays in one launch (two 64-bit counts a lane and step; the arrays start on 16-byte boundaries)
struct MutationsAbsorbJob {
  unsigned long long* into[3];
  unsigned long long* from[3];
  long long n[3];
};
__global__ void __launch_bounds__(XM_MUTATIONS_THREADS) xm_mutations_absorb_kernel(MutationsAbsorbJob job) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x, lanes = (long long)gridDim.x * blockDim.x;
  for (int a = 0; a < 3; a++) {
    const long long n = job.n[a], pairs = n >> 1;
    if (n <= 0) continue;
    ulonglong2* into2 = (ulonglong2*)job.into[a];
    ulonglong2* from2 = (ulonglong2*)job.from[a];
    for (long long i = lane; i < pairs; i += lanes) {
      const ulonglong2 f = from2[i];
      ulonglong2 t = into2[i];
      t.x += f.x; t.y += f.y;
      into2[i] = t;
      from2[i] = make_ulonglong2(0ull, 0ull);
    }
    if ((n & 1) && lane == 0) { job.into[a][n - 1] += job.from[a][n - 1]; job.from[a][n - 1] = 0ull; }
  }
}
// into[i] += staged[i] (the chunk of another GPU's counts that a peer copy brought; the source is cleared on its own GPU)
__global__ void __launch_bounds__(XM_MUTATIONS_THREADS) xm_mutations_add_kernel(unsigned long long* into, const unsigned long long* staged, long long n) {
  const long long lanes = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += lanes) into[i] += staged[i];
}

// ---------------------------------------------------------------- SNP select
struct MutationsSelectJob {
  const unsigned long long* depth;
  const unsigned long long* alt;
  long long total;
  xm::MutationFilter filter;
};

// the rows of one position as a mask over the letters; the counts it read are kept for the row (the depth is only loaded where an alt is not 0)
__device__ __forceinline__ unsigned mutationsRowsAt(const MutationsSelectJob& j, long long pos, unsigned long long alt[4], unsigned long long* depth) {
  if (pos >= j.total) return 0u;
  for (int b = 0; b < 4; b++) alt[b] = j.alt[(long long)b * j.total + pos];
  if ((alt[0] | alt[1] | alt[2] | alt[3]) == 0ull) return 0u;
  const unsigned long long d = j.depth[pos];
  *depth = d;
  unsigned mask = 0;
  for (int b = 0; b < 4; b++) if (xm::mutationsSnpRow(alt[b], d, j.filter)) mask |= 1u << b;
  return mask;
}

// pass 1: the rows of every block of XM_MUTATIONS_BLOCK positions
__global__ void __launch_bounds__(XM_MUTATIONS_THREADS) xm_mutations_count_kernel(MutationsSelectJob j, unsigned long long* blockRows) {
  __shared__ unsigned shWave[XM_MUTATIONS_THREADS / 64];
  const long long base = (long long)blockIdx.x * XM_MUTATIONS_BLOCK;
  unsigned mine = 0;
  for (int t = 0; t < XM_MUTATIONS_TILES; t++) {
    unsigned long long alt[4], depth;
    mine += __popc(mutationsRowsAt(j, base + (long long)t * XM_MUTATIONS_THREADS + threadIdx.x, alt, &depth));
  }
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
  if ((threadIdx.x & 63) == 0) shWave[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0;
    for (int w = 0; w < XM_MUTATIONS_THREADS / 64; w++) sum += shWave[w];
    blockRows[blockIdx.x] = sum;
  }
}

// The scan over the block counts, parallel at every level: the sums of every XM_MUTATIONS_SCAN_BLOCK entries of a level are the level above it, the top level
// (at most one block's worth) is scanned by one block, and every level below is scanned block by block on top of its block's offset from the level above.
__global__ void __launch_bounds__(256) xm_mutations_scan_sums_kernel(const unsigned long long* in, long long n, unsigned long long* sums) {
  __shared__ unsigned long long shWave[4];
  const long long first = (long long)blockIdx.x * XM_MUTATIONS_SCAN_BLOCK + (long long)threadIdx.x * 4;
  unsigned long long mine = 0;
  for (int k = 0; k < 4; k++) if (first + k < n) mine += in[first + k];
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
  if ((threadIdx.x & 63) == 0) shWave[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = shWave[0] + shWave[1] + shWave[2] + shWave[3];
}
// data[i] = base[block] + the sum of the block's entries in front of i (base null: 0); total (non-null only where one block covers the level): the sum of all
__global__ void __launch_bounds__(256) xm_mutations_scan_spread_kernel(unsigned long long* data, long long n, const unsigned long long* base, unsigned long long* total) {
  __shared__ unsigned long long shWave[4];
  const long long first = (long long)blockIdx.x * XM_MUTATIONS_SCAN_BLOCK + (long long)threadIdx.x * 4;
  unsigned long long v[4], mine = 0;
  for (int k = 0; k < 4; k++) { v[k] = first + k < n ? data[first + k] : 0ull; mine += v[k]; }
  unsigned long long incl = mine;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) shWave[wave] = incl;
  __syncthreads();
  unsigned long long front = base ? base[blockIdx.x] : 0ull;
  for (int w = 0; w < wave; w++) front += shWave[w];
  front += incl - mine;
  for (int k = 0; k < 4; k++) {
    if (first + k < n) data[first + k] = front;
    front += v[k];
  }
  if (total && threadIdx.x == 255) *total = front;
}

// pass 2: the rows again, each placed behind the rows of the positions in front of it and, within a position, in letter order.  blockStart: the scanned block
// counts.  A row that would land outside of rows[0 .. numRows) - the counts changed between the passes - is not written and counted in *misplaced.
__global__ void __launch_bounds__(XM_MUTATIONS_THREADS) xm_mutations_place_kernel(MutationsSelectJob j, const unsigned long long* blockStart, const int64_t* contigStart, int numContigs,
                                                                                  MutationsSnpRow* rows, unsigned long long numRows, unsigned long long* misplaced) {
  __shared__ unsigned shWave[XM_MUTATIONS_TILES][XM_MUTATIONS_THREADS / 64];
  const long long base = (long long)blockIdx.x * XM_MUTATIONS_BLOCK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long alt[XM_MUTATIONS_TILES][4], depth[XM_MUTATIONS_TILES];
  unsigned mask[XM_MUTATIONS_TILES], front[XM_MUTATIONS_TILES];
  for (int t = 0; t < XM_MUTATIONS_TILES; t++) {
    depth[t] = 0;
    mask[t] = mutationsRowsAt(j, base + (long long)t * XM_MUTATIONS_THREADS + threadIdx.x, alt[t], &depth[t]);
    const unsigned mine = __popc(mask[t]);
    unsigned incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) shWave[t][wave] = incl;
    front[t] = incl - mine;  // the rows of this wavefront's lanes in front of this one, in tile t
  }
  __syncthreads();
  unsigned before = 0;  // the rows of the block in front of (tile, wavefront), tiles first
  for (int t = 0; t < XM_MUTATIONS_TILES; t++) {
    unsigned inFront = before;
    for (int w = 0; w < XM_MUTATIONS_THREADS / 64; w++) {
      if (w < wave) inFront += shWave[t][w];
      before += shWave[t][w];
    }
    if (mask[t] == 0) continue;
    const long long pos = base + (long long)t * XM_MUTATIONS_THREADS + threadIdx.x;
    const int contig = xm::mutationsContigOf(contigStart, numContigs, pos);
    unsigned long long at = blockStart[blockIdx.x] + inFront + front[t];
    for (int b = 0; b < 4; b++) {
      if (!(mask[t] >> b & 1u)) continue;
      if (at < numRows) {
        MutationsSnpRow r;
        r.contig = contig; r.position = (int32_t)(pos - (long long)contigStart[contig]);
        r.letter = (uint8_t)b; r.referenceCode = 0;
        for (int k = 0; k < 6; k++) r.reserved[k] = 0;
        r.supportUnits = alt[t][b]; r.totalUnits = depth[t];
        rows[at] = r;
      } else {
        atomicAdd(misplaced, 1ull);
      }
      at++;
    }
  }
}

// ---------------------------------------------------------------- indel judge
// a lane per candidate; the host has checked contig, kind and length.  middle: the pile-up's middle depth (the depth itself without a query-end fraction)
__global__ void __launch_bounds__(XM_MUTATIONS_THREADS) xm_mutations_judge_kernel(const unsigned long long* middle, const int64_t* contigStart, const int32_t* contigLen,
                                                                                  xm::MutationFilter filter, const MutationsCandidate* candidates, long long n, MutationsVerdict* verdicts) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MutationsCandidate c = candidates[i];
  MutationsVerdict v;
  v.totalUnits = 0;
  v.keep = xm::mutationsJudgeIndel(middle + contigStart[c.contig], contigLen[c.contig], c.pos1, c.kind, c.length, c.supportUnits, filter, &v.totalUnits);
  verdicts[i] = v;
}

// What xm_pileup_absorb, xm_pileup_call_snps and xm_pileup_judge_indels work with (xm_capi_mutations.h): the block counts with the scan's levels above them and
// two control words (the rows in all, the rows that found no place); the contigs' starts and lengths; the rows, the candidates and their verdicts, which only
// grow; the chunk of another GPU's counts; the events of a call.  Nothing is allocated before the first of those calls.
struct MutationsStage {
  DevBuf<unsigned long long> dScan, dChunk;
  DevBuf<int64_t> dContigStart;
  DevBuf<int32_t> dContigLen;
  DevBuf<MutationsSnpRow> dRows;
  DevBuf<MutationsCandidate> dCandidates;
  DevBuf<MutationsVerdict> dVerdicts;
  StageEvents<5> ev;  // count and scan | (host sizes the rows) | place | rows down
};

}  // namespace
