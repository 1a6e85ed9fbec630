// The pile-up of the alignments on the reference (included once, by xm_capi.hip, behind xm_index): its kernel, its handle and its C entries.
#pragma once
#include "xm_pileup_text.h"
#include "xm_mutations.h"
#include "xm_indel_groups.h"

namespace {

// ---------------------------------------------------------------- pile-up of the alignments on the reference
// What MatchDatabase.addAlignments / groupByPosition feed the mutation and VCF writers with (M/Mapper.java:700-708,758-785; the classes are
// un-vendored, the behaviour is pinned by T/MatchDatabase_Test.java and T/MutationsWriter_Test.java): per forward reference position the depth
// and the counts of differing query bases, plus one event per insertion / deletion block.  One lane per query walks its result stream in HBM.
// Counts are integers in units of 1 / XM_PILEUP_UNIT of a read base (a query with n alignments adds 1/n per alignment, the two mates of a pair
// add 1/2 each where they overlap: T/MatchDatabase_Test.java:38-69), so sums do not depend on the order of the atomic adds.
struct PileupView {
  unsigned long long* depth;     // [totalForwardSize]
  unsigned long long* alt;       // [4][totalForwardSize]: query base A, C, G, T where it differs from an unambiguous reference base
  long long total;
  long long* events;             // 7 per event: contig, position, type (1 insertion, 2 deletion), length, query, mate | reversed << 1, startA; weight in [7]
  unsigned long long eventCap;
  unsigned long long* eventCount;
  long long queryBase;           // index of the batch's first query among all queries added so far
  unsigned long long* mid;       // [totalForwardSize] depth from query bases that are not near a query end (null: no query-end fraction set)
  double endFraction;            // MatchDatabase(queryEndFraction), --distinguish-query-ends (Mapper.java:76,351-353,700)
  unsigned long long* textBytes; // the bytes of text the insertion events of this call keep, summed (null: no text is kept, xm_pileup_keep_insert_text)
};
// a query base "near the end of the query": within endFraction of the query's length of either end  [inferred: the rule lives in the un-vendored
// MatchDatabase; pinned by MutationsWriter_Test.java:114-134 only for fraction 0.5 = every base]
__device__ __forceinline__ bool xmNearQueryEnd(int k, int readLen, double f) { return (double)k < f * readLen || (double)k >= readLen - f * readLen; }
__global__ void __launch_bounds__(256) xm_pileup_kernel(IndexView ix, BatchView batch, const int32_t* ints, const int64_t* intOff, PileupView pv) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= batch.nq) return;
  const int32_t* p = ints + intOff[q];
  const int numComponents = *p++;
  for (int c = 0; c < numComponents; c++) {
    const int numAlignments = *p++;
    if (numAlignments < 1) continue;
    for (int a = 0; a < numAlignments; a++) {
      // a query's alignments share one read's worth of weight exactly: UNIT / n each, the first UNIT mod n of them one unit more (n above 16 need not
      // divide UNIT; the sums over a query then still come out whole)
      const unsigned long long w = XM_PILEUP_UNIT / (unsigned long long)numAlignments + ((unsigned long long)a < XM_PILEUP_UNIT % (unsigned long long)numAlignments ? 1ull : 0ull);
      p++;  // innerDistance
      const int numSequences = *p++;
      // the reference interval of each sequence alignment first (mates of a pair share the depth where they overlap)
      int contigOf[2] = {-1, -1};
      long long lo[2] = {0, 0}, hi[2] = {0, 0};
      {
        const int32_t* t = p;
        for (int sq = 0; sq < numSequences && sq < 2; sq++) {
          contigOf[sq] = t[0];
          const int nb = t[2];
          t += 3;
          if (nb > 0) { lo[sq] = t[1]; hi[sq] = t[4 * (nb - 1) + 1] + t[4 * (nb - 1) + 3]; }
          t += 4 * nb;
        }
      }
      long long ovLo = 0, ovHi = 0;
      if (numSequences == 2 && contigOf[0] == contigOf[1]) { ovLo = lo[0] > lo[1] ? lo[0] : lo[1]; ovHi = hi[0] < hi[1] ? hi[0] : hi[1]; }
      for (int sq = 0; sq < numSequences; sq++) {
        const int contig = *p++;
        const int reversed = *p++;
        const int nb = *p++;
        const int mate = numComponents > 1 ? c : sq;
        const uint8_t* read = batch.codes + batch.mateOffset[q * 2 + mate];
        const int readLen = batch.mateLength[q * 2 + mate];
        const long long base = ix.contigStart[contig];
        for (int b = 0; b < nb; b++, p += 4) {
          const int startA = p[0], startB = p[1], lenA = p[2], lenB = p[3];
          if (lenA == lenB) {
            for (int i = 0; i < lenA; i++) {
              const long long pos = startB + i;
              const unsigned long long wi = (pos >= ovLo && pos < ovHi) ? (sq == 0 ? w / 2 : w - w / 2) : w;
              const uint8_t r = ix.refCodes[base + pos];
              const int k = startA + i;
              if (pv.mid && !xmNearQueryEnd(k, readLen, pv.endFraction)) atomicAdd(&pv.mid[base + pos], wi);
              const uint8_t qb = reversed ? bpComplement(read[readLen - 1 - k]) : read[k];
              atomicAdd(&pv.depth[base + pos], wi);
              if (!bpIsAmbiguous(r) && !bpIsAmbiguous(qb) && qb != r) atomicAdd(&pv.alt[(long long)encodedCharToInt(qb) * pv.total + base + pos], wi);
            }
          } else {
            if (lenA == 0) for (int i = 0; i < lenB; i++) {  // a deletion: the read spans these reference bases
              const long long pos = startB + i;
              const unsigned long long wi = (pos >= ovLo && pos < ovHi) ? (sq == 0 ? w / 2 : w - w / 2) : w;
              atomicAdd(&pv.depth[base + pos], wi);
              if (pv.mid && !xmNearQueryEnd(startA, readLen, pv.endFraction)) atomicAdd(&pv.mid[base + pos], wi);  // (the gap sits in front of query base startA)
            }
            const unsigned long long at = atomicAdd(pv.eventCount, 1ull);
            if (at < pv.eventCap) {
              long long* e = pv.events + at * 8;
              e[0] = contig; e[1] = startB; e[2] = lenA > 0 ? 1 : 2; e[3] = lenA > 0 ? lenA : lenB; e[4] = pv.queryBase + q; e[5] = mate | (reversed << 1) | ((pv.mid && xmNearQueryEnd(startA, readLen, pv.endFraction)) ? 4 : 0); e[6] = startA;
              e[7] = (long long)((startB >= ovLo && startB < ovHi) ? (sq == 0 ? w / 2 : w - w / 2) : w);
              if (pv.textBytes && lenA > 0) atomicAdd(pv.textBytes, (unsigned long long)pileupTextKept(1, lenA, startA, readLen));  // (the host sizes the text before the stages of xm_pileup_text.h have run)
            }
          }
        }
      }
    }
  }
}

}  // namespace

struct xm_pileup {
  xm_index* index = nullptr;            // the context whose batches are added (xm_pileup_add_last needs it alive; read / events / free do not)
  std::shared_ptr<HostShare> hs;
  int device = 0;
  DevBuf<unsigned long long> dDepth, dAlt, dEventCount, dMid;
  double endFraction = 0;
  DevBuf<long long> dEvents;
  long long total = 0, queriesAdded = 0;
  std::vector<long long> events;  // (host) 8 per event, in the order of the calls
  bool keepText = false;          // xm_pileup_keep_insert_text: the bases of every insertion event are kept beside it
  PileupTextStage textStage;      // (device) the stages' buffers
  std::vector<int64_t> textOff;   // (host) with kept text: one entry per event, plus one ...
  std::vector<char> text;         // ... into the letters of the insertions, parallel to events
  long long absorbedAt = -1;      // queriesAdded when xm_pileup_absorb last moved these counts away (-1: never, or counts came in since): nothing to move again
  MutationsStage mutations;       // (device) what xm_pileup_absorb, xm_pileup_call_snps and xm_pileup_judge_indels work with: empty until one of them is called
  bool groupEvents = false;       // xm_pileup_group_events: the events are grouped on the device; events, textOff and text above then hold the left-overs only
  IGroupsStage groups;            // (device) the table of the groups and what a fold works with: empty until the first add with grouping on
  long long eventsSeen = 0;       // with grouping: the events of all calls so far, grouped or not
};

extern "C" {

int xm_pileup_new(xm_index* idx, xm_pileup** out) {
  if (!idx || !out) return fail("xm_pileup_new: null argument");
  if (idx->hostOnly) return fail("xm_pileup_new: index was built with host_only=1");
  xm_pileup* p = nullptr;
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    HIP_CHECK(hipSetDevice(idx->device));
    p = new xm_pileup();
    p->index = idx;
    p->hs = idx->hs;
    p->device = idx->device;
    p->total = idx->host().totalForwardSize;
    p->dDepth.ensure((size_t)p->total); p->dAlt.ensure((size_t)p->total * 4); p->dEventCount.ensure(1);
    HIP_CHECK(hipMemset(p->dDepth.p, 0, sizeof(unsigned long long) * (size_t)p->total));
    HIP_CHECK(hipMemset(p->dAlt.p, 0, sizeof(unsigned long long) * (size_t)p->total * 4));
    *out = p;
    return 0;
  } catch (std::exception& e) {
    delete p;
    return fail(std::string("xm_pileup_new: ") + e.what());
  }
}

int xm_pileup_set_query_ends(xm_pileup* p, double fraction) {
  if (!p) return fail("xm_pileup_set_query_ends: null argument");
  if (!(fraction >= 0 && fraction < 1)) return fail("--distinguish-query-ends must be >= 0 and < 1");  // Mapper.java:424-425
  if (p->queriesAdded > 0) return fail("xm_pileup_set_query_ends: alignments were already added");
  try {
    HIP_CHECK(hipSetDevice(p->device));
    p->endFraction = fraction;
    if (fraction > 0) {
      p->dMid.ensure((size_t)p->total);
      HIP_CHECK(hipMemset(p->dMid.p, 0, sizeof(unsigned long long) * (size_t)p->total));
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_set_query_ends: ") + e.what()); }
}

int xm_pileup_keep_insert_text(xm_pileup* p, int32_t on) {
  if (!p) return fail("xm_pileup_keep_insert_text: null argument");
  if (p->queriesAdded > 0) return fail("xm_pileup_keep_insert_text: alignments were already added");
  try {
    HIP_CHECK(hipSetDevice(p->device));
    p->keepText = on != 0;
    if (p->keepText) p->dEventCount.ensure(2);  // (the events of a call, the bytes of their text)
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_keep_insert_text: ") + e.what()); }
}

int xm_pileup_group_events(xm_pileup* p, int32_t on) {
  if (!p) return fail("xm_pileup_group_events: null argument");
  if (p->queriesAdded > 0) return fail("xm_pileup_group_events: alignments were already added");
  try {
    HIP_CHECK(hipSetDevice(p->device));
    p->groupEvents = on != 0;
    if (p->groupEvents) {  // (grouping needs the letters: the text stage runs, and its counter is summed)
      p->keepText = true;
      p->dEventCount.ensure(2);
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_group_events: ") + e.what()); }
}

int xm_pileup_read_middle(xm_pileup* p, int32_t contig, int64_t first, int64_t n, uint64_t* depth) {
  if (!p || !p->hs || !depth) return fail("xm_pileup_read_middle: null argument");
  try {
    const HostIndex& host = p->hs->host;
    if (contig < 0 || contig >= host.numContigs() || first < 0 || n < 0 || first + n > host.contigLen[(size_t)contig]) throw std::runtime_error("range outside of the contig");
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipDeviceSynchronize());
    const size_t at = (size_t)host.contigStart[(size_t)contig] + (size_t)first;
    // (no query-end fraction: every base is a middle base)
    if (n) HIP_CHECK(hipMemcpy(depth, (p->endFraction > 0 ? p->dMid.p : p->dDepth.p) + at, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_read_middle: ") + e.what()); }
}

int xm_pileup_add_last(xm_pileup* p, int64_t* num_events) {
  if (!p || !p->index) return fail("xm_pileup_add_last: null argument");
  xm_index* idx = p->index;
  try {
    std::lock_guard<std::mutex> lock(idx->mu);
    const ResultStage::LastStreams last = lastCall(idx, "xm_pileup_add_last");
    hipStream_t s = idx->stream;
    const int64_t nq = last.nq;
    if (nq > 0) {
      const unsigned long long cap = (unsigned long long)last.intsHeld / 4 + 1;  // (an event is a block: at least four ints of the stream)
      p->dEvents.ensure((size_t)cap * 8);
      const size_t words = p->keepText ? 2 : 1;  // (with kept text the kernel also sums the bytes of it: both are read in one copy)
      HIP_CHECK(hipMemsetAsync(p->dEventCount.p, 0, sizeof(unsigned long long) * words, s));
      PileupView pv{p->dDepth.p, p->dAlt.p, p->total, p->dEvents.p, cap, p->dEventCount.p, p->queriesAdded, p->endFraction > 0 ? p->dMid.p : nullptr, p->endFraction,
                    p->keepText ? p->dEventCount.p + 1 : nullptr};
      std::shared_lock<std::shared_mutex> tablesInUse(idx->dt->rw);
      hipLaunchKernelGGL(xm_pileup_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, idx->dt->view, idx->resident.view(), last.ints, last.intOff, pv);
      HIP_CHECK(hipGetLastError());
      unsigned long long counts[2] = {0, 0};
      HIP_CHECK(hipMemcpyAsync(counts, p->dEventCount.p, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      const unsigned long long n = counts[0], textBytes = counts[1];
      if (n > cap) throw std::runtime_error("internal error: more indel events than blocks");
      if (p->groupEvents) {
        // The events are grouped where they lie (xm_indel_groups.h): the table grows first, the text stage runs without a copy or a wait of its own, and the
        // fold waits once for its small record.  Only left-overs - true fingerprint collisions - come down, in a second wait that a call without them skips.
        p->eventsSeen += (long long)n;
        if (n) {
          p->groups.reserve((long long)n, (long long)textBytes, s);
          const BatchView batch = idx->resident.view();
          const PileupTextJob job{p->dEvents.p, (long long)n, p->queriesAdded, batch.nq, batch.mateOffset, batch.mateLength, batch.codes};
          p->textStage.offsets(job, s);
          p->textStage.dText.ensure((size_t)textBytes + 1);
          if (textBytes) p->textStage.gather(job, (long long)textBytes, s);
          const IGroupsItems items{p->dEvents.p, p->textStage.dOff.p, p->textStage.dText.p, nullptr, nullptr, (long long)n};
          p->groups.fold(items, s, IGroupsLeft{&p->events, &p->textOff, &p->text});
        }
        p->queriesAdded += nq;
        if (num_events) *num_events = (int64_t)(p->events.size() / 8);
        return 0;
      }
      std::vector<long long> got((size_t)n * 8);
      std::vector<int64_t> off;
      std::vector<char> text;
      if (p->keepText && n) {  // the stages of xm_pileup_text.h over the events where they lie; a call without insertions launches no gather and copies no text
        const BatchView batch = idx->resident.view();
        const PileupTextJob job{p->dEvents.p, (long long)n, p->queriesAdded, batch.nq, batch.mateOffset, batch.mateLength, batch.codes};
        p->textStage.offsets(job, s);
        if (textBytes) p->textStage.gather(job, (long long)textBytes, s);
        off.resize((size_t)n + 1);
        text.resize((size_t)textBytes);
        HIP_CHECK(hipMemcpyAsync(off.data(), p->textStage.dOff.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
        if (textBytes) HIP_CHECK(hipMemcpyAsync(text.data(), p->textStage.dText.p, (size_t)textBytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (off[(size_t)n] != (int64_t)textBytes) throw std::runtime_error("internal error: the insertion text was measured twice with different results");
      }
      if (n) HIP_CHECK(hipMemcpy(got.data(), p->dEvents.p, sizeof(long long) * (size_t)n * 8, hipMemcpyDeviceToHost));
      // the order of the atomic appends is not fixed: events of a call are put in (query, position) order, and each one's text goes with it
      pileupAppendCall(got.data(), (size_t)n, p->keepText && n ? off.data() : nullptr, text.data(), p->events, &p->textOff, &p->text);
    }
    p->queriesAdded += nq;
    if (num_events) *num_events = (int64_t)(p->events.size() / 8);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_add_last: ") + e.what()); }
}

int xm_pileup_read(xm_pileup* p, int32_t contig, int64_t first, int64_t n, uint64_t* depth, uint64_t* alt) {
  if (!p || !p->hs || !depth || !alt) return fail("xm_pileup_read: null argument");
  try {
    const HostIndex& host = p->hs->host;  // (the pile-up shares the reference with its index: it outlives the context it was made from)
    if (contig < 0 || contig >= host.numContigs() || first < 0 || n < 0 || first + n > host.contigLen[(size_t)contig]) throw std::runtime_error("range outside of the contig");
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipDeviceSynchronize());  // (adds of a context's stream that may still be running)
    const size_t at = (size_t)host.contigStart[(size_t)contig] + (size_t)first;
    if (n) {
      HIP_CHECK(hipMemcpy(depth, p->dDepth.p + at, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
      for (int b = 0; b < 4; b++) HIP_CHECK(hipMemcpy(alt + (size_t)b * (size_t)n, p->dAlt.p + (size_t)b * (size_t)p->total + at, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_read: ") + e.what()); }
}

int64_t xm_pileup_events(xm_pileup* p, int64_t first, int64_t n, int64_t* out) {
  if (!p || (n > 0 && !out)) return -1;
  const int64_t have = (int64_t)(p->events.size() / 8);
  if (first < 0 || first > have) return -1;
  const int64_t m = std::min<int64_t>(n, have - first);
  if (m > 0) memcpy(out, p->events.data() + (size_t)first * 8, sizeof(int64_t) * (size_t)m * 8);
  return m;
}

int64_t xm_pileup_event_text(xm_pileup* p, int64_t first, int64_t n, int64_t* text_off, char* text, int64_t text_cap) {
  if (!p || !p->keepText || !text_off) return -1;
  const int64_t have = (int64_t)(p->events.size() / 8);
  const int64_t m = pileupTextPage(p->textOff, have, first, n, text_cap);
  if (m < 0) return -1;
  const int64_t base = m > 0 ? p->textOff[(size_t)first] : 0;
  for (int64_t i = 0; i <= m; i++) text_off[i] = m > 0 ? p->textOff[(size_t)(first + i)] - base : 0;
  const int64_t bytes = text_off[m];
  if (bytes > 0 && !text) return -1;
  if (bytes > 0) memcpy(text, p->text.data() + (size_t)base, (size_t)bytes);
  return m;
}

void xm_pileup_free(xm_pileup* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  delete p;
}

}  // extern "C"
