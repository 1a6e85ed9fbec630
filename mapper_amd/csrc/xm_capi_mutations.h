// xm_pileup_absorb, xm_pileup_call_snps, xm_snp_calls_free, xm_pileup_judge_indels (included once, by xm_capi.hip, behind xm_capi_pileup.h): the end of the
// mutations file made by the kernels of xm_mutations.h over the counts of a pile-up where they lie in HBM - xm_pileup_read's contract (the device is
// synchronised first, no context is needed) -, the rows copied to a pinned buffer of the library's pool.  mutationsAbsorb, mutationsSelect and mutationsJudge are
// the parts that xm_test_pileup_call (xm_capi_test.h) runs over host-given counts as well.
#pragma once

namespace {

static_assert(sizeof(xm_mutation_filter) == sizeof(xm::MutationFilter) && sizeof(xm_snp_row) == sizeof(MutationsSnpRow) &&
              sizeof(xm_indel_candidate) == sizeof(MutationsCandidate) && sizeof(xm_indel_verdict) == sizeof(MutationsVerdict), "the layouts of include/xmapper_hip.h");

xm::MutationFilter mutationsFilter(const xm_mutation_filter* f) {
  xm::MutationFilter out;
  out.minSNPTotalDepth = f->min_snp_total_depth; out.minIndelTotalStartDepth = f->min_indel_total_start_depth;
  out.minIndelContinuationTotalDepth = f->min_indel_continuation_total_depth;
  out.minSNPDepthFraction = f->min_snp_depth_fraction; out.minIndelStartDepthFraction = f->min_indel_start_depth_fraction;
  out.minIndelContinuationDepthFraction = f->min_indel_continuation_depth_fraction;
  out.reserved = 0;
  return out;
}

// xm_snp_calls plus what xm_snp_calls_free needs to know about its buffer
struct SnpBox {
  xm_snp_calls pub;
  size_t bytesRows;
};

void freeSnpBox(SnpBox* box) {
  g_pinned->put(box->pub.rows, box->bytesRows);
  free(box);
}

unsigned mutationsGrid(long long n) {  // a grid-stride launch over n elements: enough blocks to fill the GPU, never more than the elements ask for
  const long long blocks = (n + XM_MUTATIONS_THREADS - 1) / XM_MUTATIONS_THREADS;
  return (unsigned)std::max<long long>(1, std::min<long long>(blocks, 8192));
}

// into += from, from = 0 on the current GPU, on stream s (both sets have a middle depth or neither has)
void mutationsAbsorb(const MutationsCounts& into, const MutationsCounts& from, hipStream_t s) {
  if (into.total <= 0) return;
  MutationsAbsorbJob job;
  job.into[0] = into.depth; job.from[0] = from.depth; job.n[0] = into.total;
  job.into[1] = into.alt; job.from[1] = from.alt; job.n[1] = into.total * 4;
  job.into[2] = into.mid; job.from[2] = from.mid; job.n[2] = into.mid ? into.total : 0;
  hipLaunchKernelGGL(xm_mutations_absorb_kernel, dim3(mutationsGrid(into.total * 2)), dim3(XM_MUTATIONS_THREADS), 0, s, job);
  HIP_CHECK(hipGetLastError());
}

// The same from another GPU: chunk by chunk a peer copy into g.dChunk on into's GPU (the current one), the add there, and the clear at the source.
constexpr long long XM_MUTATIONS_CHUNK = 4ll << 20;  // counts a chunk (32 MiB)
void mutationsAbsorbPeer(MutationsStage& g, const MutationsCounts& into, int intoDevice, const MutationsCounts& from, int fromDevice) {
  if (into.total <= 0) return;
  g.dChunk.ensure((size_t)std::min<long long>(XM_MUTATIONS_CHUNK, into.total * 4));
  unsigned long long* intoOf[3] = {into.depth, into.alt, into.mid};
  unsigned long long* fromOf[3] = {from.depth, from.alt, from.mid};
  const long long nOf[3] = {into.total, into.total * 4, into.mid ? into.total : 0};
  for (int a = 0; a < 3; a++)
    for (long long at = 0; at < nOf[a]; at += XM_MUTATIONS_CHUNK) {
      const long long n = std::min<long long>(XM_MUTATIONS_CHUNK, nOf[a] - at);
      HIP_CHECK(hipMemcpyPeer(g.dChunk.p, intoDevice, fromOf[a] + at, fromDevice, sizeof(unsigned long long) * (size_t)n));
      hipLaunchKernelGGL(xm_mutations_add_kernel, dim3(mutationsGrid(n)), dim3(XM_MUTATIONS_THREADS), 0, nullptr, intoOf[a] + at, (const unsigned long long*)g.dChunk.p, n);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());  // (the chunk is free for the next copy, and what was added is cleared only once it was added)
      HIP_CHECK(hipSetDevice(fromDevice));
      HIP_CHECK(hipMemset(fromOf[a] + at, 0, sizeof(unsigned long long) * (size_t)n));
      HIP_CHECK(hipDeviceSynchronize());
      HIP_CHECK(hipSetDevice(intoDevice));
    }
}

// the contigs' starts and lengths in HBM (a few bytes a contig, copied up by every call: a pile-up has no context to borrow them from)
void mutationsContigs(MutationsStage& g, const int64_t* start, const int32_t* len, int numContigs, hipStream_t s) {
  g.dContigStart.ensure((size_t)numContigs); g.dContigLen.ensure((size_t)numContigs);
  HIP_CHECK(hipMemcpyAsync(g.dContigStart.p, start, sizeof(int64_t) * (size_t)numContigs, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(g.dContigLen.p, len, sizeof(int32_t) * (size_t)numContigs, hipMemcpyHostToDevice, s));
}

// The select on stream s over counts in HBM.  Returns the rows in a pinned buffer (rows null when there are none: nothing is launched behind the total), or throws.
SnpBox* mutationsSelect(MutationsStage& g, const MutationsCounts& c, const int64_t* contigStart, const int32_t* contigLen, int numContigs, const xm::MutationFilter& f, hipStream_t s) {
  SnpBox* box = (SnpBox*)calloc(1, sizeof(SnpBox));
  if (!box) throw std::runtime_error("out of host memory");
  box->pub.store = box;
  box->pub.positions = c.total;
  if (c.total <= 0) return box;  // (nothing is launched)
  try {
    g.ev.ready();
    // the levels of the scan: the block counts, then the sums of every XM_MUTATIONS_SCAN_BLOCK entries of the level below, up to a level one block covers
    std::vector<long long> levelN, levelAt;
    long long words = 0;
    for (long long n = (c.total + XM_MUTATIONS_BLOCK - 1) / XM_MUTATIONS_BLOCK;; n = (n + XM_MUTATIONS_SCAN_BLOCK - 1) / XM_MUTATIONS_SCAN_BLOCK) {
      levelN.push_back(n); levelAt.push_back(words);
      words += n;
      if (n <= XM_MUTATIONS_SCAN_BLOCK) break;
    }
    const int top = (int)levelN.size() - 1;
    g.dScan.ensure((size_t)words + 2);  // (a buffer that grows frees the old one, which waits for the device: before anything is queued)
    unsigned long long* ctl = g.dScan.p + words;  // [rows in all, rows that found no place]
    mutationsContigs(g, contigStart, contigLen, numContigs, s);
    const MutationsSelectJob job{c.depth, c.alt, c.total, f};
    HIP_CHECK(hipEventRecord(g.ev[0], s));
    HIP_CHECK(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 2, s));
    hipLaunchKernelGGL(xm_mutations_count_kernel, dim3((unsigned)levelN[0]), dim3(XM_MUTATIONS_THREADS), 0, s, job, g.dScan.p);
    for (int k = 0; k < top; k++)
      hipLaunchKernelGGL(xm_mutations_scan_sums_kernel, dim3((unsigned)levelN[(size_t)k + 1]), dim3(256), 0, s, (const unsigned long long*)(g.dScan.p + levelAt[(size_t)k]), levelN[(size_t)k],
                         g.dScan.p + levelAt[(size_t)k + 1]);
    hipLaunchKernelGGL(xm_mutations_scan_spread_kernel, dim3(1), dim3(256), 0, s, g.dScan.p + levelAt[(size_t)top], levelN[(size_t)top], (const unsigned long long*)nullptr, ctl);
    for (int k = top - 1; k >= 0; k--)
      hipLaunchKernelGGL(xm_mutations_scan_spread_kernel, dim3((unsigned)levelN[(size_t)k + 1]), dim3(256), 0, s, g.dScan.p + levelAt[(size_t)k], levelN[(size_t)k],
                         (const unsigned long long*)(g.dScan.p + levelAt[(size_t)k + 1]), (unsigned long long*)nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(g.ev[1], s));
    unsigned long long got[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(&got[0], ctl, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (the one wait for the total)
    const size_t nRows = (size_t)got[0];
    float count = 0, place = 0, down = 0;
    HIP_CHECK(hipEventElapsedTime(&count, g.ev[0], g.ev[1]));
    box->pub.num_rows = (int64_t)nRows;
    box->pub.bytes_to_host = (int64_t)sizeof(unsigned long long);
    if (nRows) {
      g.dRows.ensure(nRows);
      box->pub.rows = (xm_snp_row*)g_pinned->get(sizeof(xm_snp_row) * nRows, &box->bytesRows);
      HIP_CHECK(hipEventRecord(g.ev[2], s));
      HIP_CHECK(hipMemsetAsync(g.dRows.p, 0, sizeof(MutationsSnpRow) * nRows, s));  // (a row that no lane writes - the counts changed between the passes - must not be garbage)
      hipLaunchKernelGGL(xm_mutations_place_kernel, dim3((unsigned)levelN[0]), dim3(XM_MUTATIONS_THREADS), 0, s, job, (const unsigned long long*)g.dScan.p, (const int64_t*)g.dContigStart.p, numContigs,
                         g.dRows.p, (unsigned long long)nRows, ctl + 1);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(g.ev[3], s));
      HIP_CHECK(hipMemcpyAsync(box->pub.rows, g.dRows.p, sizeof(MutationsSnpRow) * nRows, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(&got[1], ctl + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipEventRecord(g.ev[4], s));
      HIP_CHECK(hipEventSynchronize(g.ev[4]));
      if (got[1] != 0) throw std::runtime_error("internal error: " + std::to_string(got[1]) + " rows found no place (the counts changed between the two passes)");
      HIP_CHECK(hipEventElapsedTime(&place, g.ev[2], g.ev[3]));
      HIP_CHECK(hipEventElapsedTime(&down, g.ev[3], g.ev[4]));
      box->pub.bytes_to_host += (int64_t)(sizeof(MutationsSnpRow) * nRows + sizeof(unsigned long long));
    }
    box->pub.kernel_ms = (double)count + place; box->pub.d2h_ms = down;
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);  // (nothing of this call is still in flight when its buffers go)
    freeSnpBox(box);
    throw;
  }
}

// The judge on stream s: n >= 1 candidates that the caller has checked (mutationsCheckCandidates) against the contigs that are copied up here.
void mutationsJudge(MutationsStage& g, const MutationsCounts& c, const int64_t* contigStart, const int32_t* contigLen, int numContigs, const xm::MutationFilter& f,
                    const xm_indel_candidate* candidates, int64_t n, xm_indel_verdict* verdicts, hipStream_t s) {
  g.dCandidates.ensure((size_t)n); g.dVerdicts.ensure((size_t)n);
  mutationsContigs(g, contigStart, contigLen, numContigs, s);
  HIP_CHECK(hipMemcpyAsync(g.dCandidates.p, candidates, sizeof(MutationsCandidate) * (size_t)n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(xm_mutations_judge_kernel, dim3((unsigned)((n + XM_MUTATIONS_THREADS - 1) / XM_MUTATIONS_THREADS)), dim3(XM_MUTATIONS_THREADS), 0, s,
                     (const unsigned long long*)(c.mid ? c.mid : c.depth), (const int64_t*)g.dContigStart.p, (const int32_t*)g.dContigLen.p, f, (const MutationsCandidate*)g.dCandidates.p,
                     (long long)n, g.dVerdicts.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(verdicts, g.dVerdicts.p, sizeof(MutationsVerdict) * (size_t)n, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

void mutationsCheckCandidates(const xm_indel_candidate* candidates, int64_t n, const int32_t* contigLen, int numContigs) {
  for (int64_t i = 0; i < n; i++) {
    const xm_indel_candidate& c = candidates[i];
    if (c.contig < 0 || c.contig >= numContigs) throw std::runtime_error("candidate " + std::to_string(i) + ": contig outside of the reference");
    if (contigLen[c.contig] < 1) throw std::runtime_error("candidate " + std::to_string(i) + ": its contig has no bases");
    if (c.kind != 1 && c.kind != 2) throw std::runtime_error("candidate " + std::to_string(i) + ": kind must be 1 (insertion) or 2 (deletion)");
  }
}

MutationsCounts mutationsCountsOf(xm_pileup* p) { return MutationsCounts{p->dDepth.p, p->dAlt.p, p->endFraction > 0 ? p->dMid.p : nullptr, p->total}; }

// ---------------------------------------------------------------- the groups of xm_indel_groups.h at the end
static_assert(sizeof(xm_indel_call) == sizeof(IGroupsCall), "the layouts of include/xmapper_hip.h");

// xm_indel_calls plus what xm_indel_calls_free needs to know about its buffers
struct IndelBox {
  xm_indel_calls pub;
  size_t bytesRows, bytesLetters;
};

void freeIndelBox(IndelBox* box) {
  if (box->pub.rows) g_pinned->put(box->pub.rows, box->bytesRows);
  if (box->pub.letters) g_pinned->put(box->pub.letters, box->bytesLetters);
  free(box);
}

// The groups of g judged over `middle` (null: no counts - every group comes down whole with a total of 0) on stream s: a lane per group, two scans over the
// kept ones and their letters, and the records and letters gathered into pinned buffers.  f null: unjudged.  Two waits: the totals, then the records.
IndelBox* igroupsCall(IGroupsStage& g, MutationsStage& m, const unsigned long long* middle, const int64_t* contigStart, const int32_t* contigLen, int numContigs, const xm::MutationFilter* f,
                      hipStream_t s) {
  IndelBox* box = (IndelBox*)calloc(1, sizeof(IndelBox));
  if (!box) throw std::runtime_error("out of host memory");
  box->pub.store = box;
  box->pub.groups = g.groups;
  const long long n = g.groups;
  if (n <= 0) return box;  // (nothing is launched)
  try {
    g.dKeep.ensure((size_t)n); g.dTotal.ensure((size_t)n); g.dFlag.ensure((size_t)n); g.dLen.ensure((size_t)n); g.dBlocks.ensure(xmScanSums(n, 1));
    g.dOffA.ensure((size_t)n + 1); g.dOffB.ensure((size_t)n + 1);
    if (middle) mutationsContigs(m, contigStart, contigLen, numContigs, s);
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(xm_igroups_judge_kernel, dim3(grid), dim3(256), 0, s, (const xm::IndelGroup*)g.dGroups.p, n, middle, (const int64_t*)m.dContigStart.p, (const int32_t*)m.dContigLen.p,
                       middle ? numContigs : 0, f ? *f : xm::MutationFilter{0, 0, 0, 0, 0, 0, 0}, f ? 1 : 0, g.dKeep.p, g.dTotal.p, g.dFlag.p, g.dLen.p);
    HIP_CHECK(hipGetLastError());
    xmScan(XmOffsets<long long, 1>{n, {g.dFlag.p}, {g.dOffA.p}}, n, g.dBlocks, s);
    xmScan(XmOffsets<long long, 1>{n, {g.dLen.p}, {g.dOffB.p}}, n, g.dBlocks, s);
    int64_t totals[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(&totals[0], g.dOffA.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&totals[1], g.dOffB.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t kept = (size_t)totals[0], letters = (size_t)totals[1];
    box->pub.num_rows = (int64_t)kept;
    box->pub.num_letters = (int64_t)letters;
    box->pub.bytes_to_host = (int64_t)sizeof(totals);
    if (kept) {
      g.dCalls.ensure(kept); g.dLeftText.ensure(letters + 1);
      box->pub.rows = (xm_indel_call*)g_pinned->get(sizeof(xm_indel_call) * kept, &box->bytesRows);
      if (letters) box->pub.letters = (char*)g_pinned->get(letters, &box->bytesLetters);
      hipLaunchKernelGGL(xm_igroups_gather_kernel, dim3(grid), dim3(256), 0, s, (const xm::IndelGroup*)g.dGroups.p, (const char*)g.dArena.p, n, (const long long*)g.dKeep.p,
                         (const unsigned long long*)g.dTotal.p, (const long long*)g.dFlag.p, (const int64_t*)g.dOffA.p, (const int64_t*)g.dOffB.p, g.dCalls.p, (long long)kept, g.dLeftText.p,
                         (long long)letters);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(box->pub.rows, g.dCalls.p, sizeof(IGroupsCall) * kept, hipMemcpyDeviceToHost, s));
      if (letters) HIP_CHECK(hipMemcpyAsync(box->pub.letters, g.dLeftText.p, letters, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      box->pub.bytes_to_host += (int64_t)(sizeof(IGroupsCall) * kept + letters);
    }
    return box;
  } catch (...) {
    (void)hipStreamSynchronize(s);
    freeIndelBox(box);
    throw;
  }
}

// The groups of `from` folded into `into`'s table as items, and `from`'s table emptied; what the fold leaves over goes to `left` as events.  Both branches
// are "compact, (copy,) fold": the records and the used part of the arena are compacted into staging buffers on from's GPU, brought to into's GPU by peer copy
// when that is another one, and folded there by the kernels every add runs.  The current GPU is into's, before and after.
void igroupsAbsorb(IGroupsStage& into, int intoDevice, IGroupsStage& from, int fromDevice, const IGroupsLeft& left) {
  const long long n = from.groups;
  if (n <= 0) return;
  const long long bytes = from.arenaUsed;
  HIP_CHECK(hipSetDevice(fromDevice));
  DevBuf<xm::IndelGroup> staged;
  DevBuf<char> stagedArena;
  staged.ensure((size_t)n); stagedArena.ensure((size_t)bytes + 8);
  HIP_CHECK(hipMemcpy(staged.p, from.dGroups.p, sizeof(xm::IndelGroup) * (size_t)n, hipMemcpyDeviceToDevice));
  if (bytes) HIP_CHECK(hipMemcpy(stagedArena.p, from.dArena.p, (size_t)bytes, hipMemcpyDeviceToDevice));
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipSetDevice(intoDevice));
  DevBuf<xm::IndelGroup> here;
  DevBuf<char> hereArena;
  const xm::IndelGroup* records = staged.p;
  const char* arena = stagedArena.p;
  if (intoDevice != fromDevice) {
    here.ensure((size_t)n); hereArena.ensure((size_t)bytes + 8);
    HIP_CHECK(hipMemcpyPeer(here.p, intoDevice, staged.p, fromDevice, sizeof(xm::IndelGroup) * (size_t)n));
    if (bytes) HIP_CHECK(hipMemcpyPeer(hereArena.p, intoDevice, stagedArena.p, fromDevice, (size_t)bytes));
    records = here.p; arena = hereArena.p;
  }
  into.reserve(n, bytes, nullptr);
  into.fold(IGroupsItems{nullptr, nullptr, nullptr, records, arena, n}, nullptr, left);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipSetDevice(fromDevice));
  from.clear(nullptr);
  HIP_CHECK(hipDeviceSynchronize());
  staged = DevBuf<xm::IndelGroup>(); stagedArena = DevBuf<char>();  // (freed on the GPU they were made on)
  HIP_CHECK(hipSetDevice(intoDevice));
}

}  // namespace

extern "C" {

int64_t xm_mutations_block_positions(void) { return XM_MUTATIONS_BLOCK; }

int xm_pileup_absorb(xm_pileup* into, xm_pileup* from) {
  if (!into || !from) return fail("xm_pileup_absorb: null argument");
  if (into == from) return fail("xm_pileup_absorb: the same pile-up was given twice");
  if (!into->hs || into->hs != from->hs || into->total != from->total) return fail("xm_pileup_absorb: the pile-ups belong to different indexes");
  if (into->endFraction != from->endFraction) return fail("xm_pileup_absorb: the pile-ups have different query-end fractions");
  if (into->groupEvents != from->groupEvents) return fail("xm_pileup_absorb: one pile-up groups its events on the device (xm_pileup_group_events) and the other does not");
  if (from->absorbedAt == from->queriesAdded) return 0;  // (its counts were moved away and none came since: every count is 0)
  try {
    if (into->device != from->device) {
      int can = 0;
      HIP_CHECK(hipDeviceCanAccessPeer(&can, into->device, from->device));
      if (!can) throw std::runtime_error("GPU " + std::to_string(into->device) + " cannot reach GPU " + std::to_string(from->device) + " by peer copy");
      HIP_CHECK(hipSetDevice(from->device));
      HIP_CHECK(hipDeviceSynchronize());
    }
    HIP_CHECK(hipSetDevice(into->device));
    HIP_CHECK(hipDeviceSynchronize());  // (adds of the contexts' streams that may still be running)
    if (into->device == from->device) {
      mutationsAbsorb(mutationsCountsOf(into), mutationsCountsOf(from), nullptr);
      HIP_CHECK(hipDeviceSynchronize());
    } else {
      mutationsAbsorbPeer(into->mutations, mutationsCountsOf(into), into->device, mutationsCountsOf(from), from->device);
    }
    if (into->groupEvents) igroupsAbsorb(into->groups, into->device, from->groups, from->device, IGroupsLeft{&into->events, &into->textOff, &into->text});
    from->absorbedAt = from->queriesAdded;
    into->absorbedAt = -1;
    return 0;
  } catch (std::exception& e) {
    (void)hipSetDevice(into->device);
    return fail(std::string("xm_pileup_absorb: ") + e.what());
  }
}

int xm_pileup_call_snps(xm_pileup* p, const xm_mutation_filter* filter, xm_snp_calls** out) {
  if (!p || !p->hs || !filter || !out) return fail("xm_pileup_call_snps: null argument");
  *out = nullptr;
  try {
    const HostIndex& host = p->hs->host;
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipDeviceSynchronize());
    SnpBox* box = mutationsSelect(p->mutations, mutationsCountsOf(p), host.contigStart.data(), host.contigLen.data(), host.numContigs(), mutationsFilter(filter), nullptr);
    for (int64_t i = 0; i < box->pub.num_rows; i++) {  // (the reference is host memory of the index: the rows are few)
      xm_snp_row& r = box->pub.rows[i];
      r.reference_code = host.refCodes[(size_t)host.contigStart[(size_t)r.contig] + (size_t)r.position];
    }
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_call_snps: ") + e.what()); }
}

void xm_snp_calls_free(xm_snp_calls* calls) {
  if (calls) freeSnpBox((SnpBox*)calls);  // pub is the first member
}

int xm_pileup_call_indels(xm_pileup* p, const xm_mutation_filter* filter, xm_indel_calls** out) {
  if (!p || !p->hs || !out) return fail("xm_pileup_call_indels: null argument");
  *out = nullptr;
  if (!p->groupEvents) return fail("xm_pileup_call_indels: the pile-up does not group its events on the device (xm_pileup_group_events)");
  try {
    const HostIndex& host = p->hs->host;
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipDeviceSynchronize());
    xm::MutationFilter f;
    if (filter) f = mutationsFilter(filter);
    const MutationsCounts c = mutationsCountsOf(p);
    IndelBox* box = igroupsCall(p->groups, p->mutations, c.mid ? c.mid : c.depth, host.contigStart.data(), host.contigLen.data(), host.numContigs(), filter ? &f : nullptr, nullptr);
    box->pub.events = p->eventsSeen;
    box->pub.left_over = (int64_t)(p->events.size() / 8);
    box->pub.table_bytes = (int64_t)(p->groups.cap * 16 + p->groups.dGroups.n * sizeof(xm::IndelGroup) + p->groups.dArena.n);
    *out = &box->pub;
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_call_indels: ") + e.what()); }
}

void xm_indel_calls_free(xm_indel_calls* calls) {
  if (calls) freeIndelBox((IndelBox*)calls);  // pub is the first member
}

int xm_pileup_judge_indels(xm_pileup* p, const xm_mutation_filter* filter, const xm_indel_candidate* candidates, int64_t n, xm_indel_verdict* verdicts) {
  if (!p || !p->hs || !filter) return fail("xm_pileup_judge_indels: null argument");
  if (n < 0) return fail("xm_pileup_judge_indels: negative size");
  if (n == 0) return 0;  // (nothing is launched)
  if (!candidates || !verdicts) return fail("xm_pileup_judge_indels: null argument");
  try {
    const HostIndex& host = p->hs->host;
    mutationsCheckCandidates(candidates, n, host.contigLen.data(), host.numContigs());
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipDeviceSynchronize());
    mutationsJudge(p->mutations, mutationsCountsOf(p), host.contigStart.data(), host.contigLen.data(), host.numContigs(), mutationsFilter(filter), candidates, n, verdicts, nullptr);
    return 0;
  } catch (std::exception& e) { return fail(std::string("xm_pileup_judge_indels: ") + e.what()); }
}

}  // extern "C"
