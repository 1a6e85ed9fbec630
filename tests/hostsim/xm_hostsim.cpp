// HOST SIMULATION OF THE DEVICE KERNEL — TEST HARNESS ONLY.
//
// There is no GPU in the development container, so the kernel sources (mapper_amd/csrc/xm_*.h) are also compiled for the
// host here and driven read by read, exactly as a lane of xm_align_kernel would, to let the CPU-only test tier compare the
// kernel logic with the oracle.  This file is built by tests/ into tests/_build/libxm_hostsim.so; it is never linked into
// or loaded by libxmapper_hip.so / the mapper_amd package, which has no CPU path.
#include "../../include/xmapper_hip.h"
#include "../../mapper_amd/csrc/xm_worker.h"
#include "../../mapper_amd/csrc/xm_wsearch.h"
#include "../../mapper_amd/csrc/xm_wave.h"
#include "../../mapper_amd/csrc/xm_index_host.h"
#include "../../mapper_amd/csrc/xm_pass_plan.h"
#include "../../mapper_amd/csrc/xm_conf_table.h"
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace xm;

// XM_ARENA_TRACE builds (scripts/light_pass_footprint.py): the allocations of the arenas, in order
#if defined(XM_ARENA_TRACE)
struct ArenaAlloc { const void* base; size_t offset, bytes; };
static std::vector<ArenaAlloc> g_allocs;
static bool g_traceOn = false;
namespace xm { void xm_arena_trace(const void* base, size_t offset, size_t bytes) { if (g_traceOn) g_allocs.push_back(ArenaAlloc{base, offset, bytes}); } }
#endif

static thread_local std::string g_err;
static int g_waveMode = -1;  // -1: from XMSIM_WAVE (default 0)
static long long g_waveStatus[16];
static long long g_waveWhy[64];
static long long g_markHist[6][128];  // high-water marks of the wave form per read: chunks, counters, history, pending, query matches, alignments
static void markDump() { const char* names[6] = {"chunks", "counters", "history", "pending", "qmatches", "alignments"}; for (int k = 0; k < 6; k++) { fprintf(stderr, "[wave marks] %s:", names[k]); for (int i = 0; i < 128; i++) if (g_markHist[k][i]) fprintf(stderr, " %d:%lld", i, g_markHist[k][i]); fprintf(stderr, "\n"); } }

struct SimIndex {
  HostIndex host;
  IndexView view;
  int32_t baSteps[24];
  std::vector<uint32_t> p32, l32;
  std::vector<uint64_t> l64;
  void refresh() {
    bool is64 = host.seqCumStart.back() > 0xFFFFFFFFll;
    p32.clear();
    if (!is64) { p32.resize(host.positions.size()); for (size_t i = 0; i < p32.size(); i++) p32[i] = (uint32_t)host.positions[i]; }
    fillHostFields(view, host, is64);
    view.contigStart = host.contigStart.data(); view.contigLen = host.contigLen.data(); view.seqCumStart = host.seqCumStart.data(); view.refCodes = host.refCodes.data();
    view.tables = host.tables.data(); view.bucketOff = host.bucketOff.data(); view.positions32 = p32.data(); view.positions64 = (const uint64_t*)host.positions.data();
    view.dupKeyStart = host.dupKeyStart.data(); view.dupKeys = host.dupKeys.data();
    view.conf = nullptr; view.confMask = 0; view.confMiss = nullptr;   // (the host simulation evaluates the confidence term in place: xm_worker.h)
    blockAlignerLogSteps(baSteps, 24);
    view.baLogStep = baSteps;
    // bucket lines (IndexView::lines32 / lines64), filled by the function the device kernel uses; XMSIM_LINES=0: CSR probes only
    view.lines32 = nullptr; view.lines64 = nullptr;
    l32.clear(); l64.clear();
    const char* le = getenv("XMSIM_LINES");
    if (!(le && *le && atoi(le) == 0)) {
      if (is64) l64.assign(host.bucketOff.size() * 8, 0); else l32.assign(host.bucketOff.size() * 8, 0);
      for (const Table& t : host.tables)
        for (int64_t k = 0; k < t.capacity; k++) {
          const uint32_t* off = host.bucketOff.data() + t.offBase + k;
          if (is64) xmFillLine(l64.data() + (t.offBase + k) * 8, off[0], off[1], (const uint64_t*)host.positions.data() + t.posBase);
          else xmFillLine(l32.data() + (t.offBase + k) * 8, off[0], off[1], p32.data() + t.posBase);
        }
      view.lines32 = is64 ? nullptr : l32.data(); view.lines64 = is64 ? l64.data() : nullptr;
    }
  }
};

extern "C" {

const char* xmsim_last_error() { return g_err.c_str(); }

void* xmsim_index_build(const xm_ref* ref, const xm_build_opts* o) {
  try {
    SimIndex* s = new SimIndex();
    s->host.setReference(ref->num_contigs, ref->names, ref->codes, ref->lengths);
    s->host.build(o->enable_gapmers, o->min_interesting_size, o->max_hashed_length, o->dup_window, o->dup_min_copies, o->dup_min_length, o->dup_max_length);
    s->refresh();
    return s;
  } catch (std::exception& e) { g_err = e.what(); return nullptr; }
}
void xmsim_index_free(void* p) { delete (SimIndex*)p; }

// same result layout as xm_align_batch; counters[11] = reads rerun at a larger scale; returns non-zero on failure
int xmsim_align_batch(void* idxp, const xm_params* p, const xm_query_batch* b, xm_result** out) {
  SimIndex* idx = (SimIndex*)idxp;
  try {
    int maxLen = 1;
    for (int64_t q = 0; q < b->num_queries; q++) for (int m = 0; m < b->mate_count[q]; m++) if (b->mate_length[q * 2 + m] > maxLen) maxLen = b->mate_length[q * 2 + m];
    if (maxLen > idx->host.maxHashedLength) { idx->host.ensureLength(maxLen); idx->refresh(); }
    const Params params = paramsFromC(*p);
    const int64_t nq = b->num_queries;
    std::vector<int32_t> ints;
    std::vector<double> dbls;
    xm_result* res = (xm_result*)calloc(1, sizeof(xm_result));
    res->num_queries = nq;
    res->int_off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nq + 1));
    res->dbl_off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nq + 1));
    DevCounters dc;
    memset(&dc, 0, sizeof(dc));
    int64_t rerun = 0;
    std::vector<uint8_t> arena;
    static ReadCtx cx;  // large; keep it off the stack
    for (int64_t q = 0; q < nq; q++) {
      ReadIn in;
      in.nMates = b->mate_count[q];
      for (int m = 0; m < 2; m++) { in.mate[m] = b->codes + b->mate_offset[q * 2 + m]; in.mateLen[m] = m < in.nMates ? b->mate_length[q * 2 + m] : 0; }
      in.expectedInner = in.nMates > 1 ? b->expected_inner[q] : 0.0;
      in.deviation = in.nMates > 1 ? b->deviation[q] : 1.0;
      // the wave-per-read form first (XMSIM_WAVE: 1 = its light tier, 2 = light then heavy tier), exactly as the product's passes 0 / 0b run
      // it (mapper_amd/csrc/xm_wave.h; a WV_PAR region is a loop over the 64 lanes here); reads it does not finish go through the
      // lane-per-read sequence below
      const int waveMode = g_waveMode >= 0 ? g_waveMode : (getenv("XMSIM_WAVE") ? atoi(getenv("XMSIM_WAVE")) : 0);
      if (waveMode > 0) {
        typedef WaveLdsT<WCfgLightPE> LightLds;
        typedef WaveLdsT<WCfgMidPE> MidLds;
        typedef WaveLdsT<WCfgHeavy> HeavyLds;
        static LightLds ldsLight;
        static MidLds ldsMid;
        static HeavyLds ldsHeavy;
        static std::vector<uint8_t> waveArena((size_t)(XM_ARENA_KB_DEFAULT * 1024 * 4 * 7 / 12 + 4096));
        static WMemo memo;
        memo.count = 0; memo.pending = 0;
        bool finished = false;
        int searchRounds = 0;
        // waveMode 1: light tier only; 2: + chain tier (with its search rounds); 3: + the chain tier with the largest capacities
        for (int tier = 0; tier < waveMode && tier < 3 && !finished; ) {
          DevCounters before = dc;
          WEnv e;
          e.ix = idx->view; e.params = params; e.dc = &dc; e.mateBase[0] = in.mate[0]; e.mateBase[1] = in.mate[1]; e.tier = tier;
          Caps caps = makeCaps(4);
          caps.heavyAllowed = 2;
          Arena tmp;
          tmp.init((void*)(((uintptr_t)waveArena.data() + 15) & ~(uintptr_t)15), waveArena.size() - 64);
          e.caps = &caps; e.tmp = &tmp;
          e.memo = tier == 0 ? nullptr : &memo;
          static std::vector<WSNode> inlineNodes(WSearchLdsInline::kNodes);
          static const bool inlineSearch = !(getenv("XMSIM_NO_INLINE_SEARCH") && atoi(getenv("XMSIM_NO_INLINE_SEARCH")) != 0);  // (0: every search through the memo and the search "kernel")
          e.searchNodes = tier == 0 || !inlineSearch ? nullptr : inlineNodes.data();
          WResult wr;
          int32_t st = 0, why = 0;
          int64_t ni = 0, nd = 0;
          auto run = [&](auto& Ld) {
            wAlignRead(&Ld, e, in, wr);
            st = Ld.status; why = Ld.why;
            if (st == XM_OK) wResultSize(&Ld, wr, ni, nd);
            if (getenv("XMSIM_WAVE_STATS")) {
              static bool reg = false; if (!reg) { reg = true; atexit(markDump); }
              auto clip = [](int v) { return v < 0 ? 0 : (v > 127 ? 127 : v); };
              g_markHist[0][clip(Ld.nChunksUsed)]++;
              for (int m = 0; m < in.nMates; m++) { g_markHist[1][clip(Ld.m[m].nCounters)]++; g_markHist[2][clip(Ld.m[m].nHistory)]++; g_markHist[3][clip(Ld.m[m].pendTail)]++; }
              g_markHist[4][clip(Ld.nAssembled)]++; g_markHist[5][clip(Ld.al[0].nGood)]++;
            }
          };
          auto write = [&](auto& Ld) { wResultWrite(&Ld, wr, ints.data() + res->int_off[q], dbls.data() + res->dbl_off[q], &dc); };
          if (tier == 0) run(ldsLight); else if (tier == 1) run(ldsMid); else run(ldsHeavy);
          g_waveStatus[st < 16 ? st : 15]++;
          if (st == XM_ST_WAVE_FALLBACK || (st == XM_ST_WAVE_GAPPED && tier >= 1)) g_waveWhy[why & 63]++;
          if (st == XM_OK) {
            res->int_off[q] = (int64_t)ints.size(); res->dbl_off[q] = (int64_t)dbls.size();
            ints.resize(ints.size() + (size_t)ni); dbls.resize(dbls.size() + (size_t)nd);
            if (tier == 0) write(ldsLight); else if (tier == 1) write(ldsMid); else write(ldsHeavy);
            finished = true;
          } else {
            dc = before;
            if (st == XM_ST_WAVE_SEARCH) {  // the search "kernel", then the same tier again
              const int mi = memo.req.seqAId >> 1;
              static WSearchLdsKernel searchLds;
              static std::vector<WSNode> searchNodes(WSearchLdsKernel::kNodes);
              wRunSearch(&searchLds, searchNodes.data(), idx->view, params, in.mate[mi], in.mateLen[mi], &memo);
              if (++searchRounds > 4 * WV_MEMO_MAX) throw std::runtime_error("search rounds do not end");
              continue;
            }
            if (st != XM_ST_WAVE_FALLBACK && st != XM_ST_WAVE_GAPPED) throw std::runtime_error("Failed to align query " + std::to_string(q) + " (wave status " + std::to_string(st) + ")");
            if (st == XM_ST_WAVE_FALLBACK) break;  // (ambiguity codes, long or overlapping mates: no tier of the wave form takes them)
            tier++;
          }
        }
        if (finished) continue;
      }
      // the product's pass sequence for one read (xm_pass_plan.h, PassState / nextPass, with a work list of this one read): light pass at the seed scale; a read
      // that needs the gapped chain goes on at the gapped scale from the state it saved (hand-over), on another context object and other temporaries; scratch
      // overflow -> reruns from the start at four times the scale.  XMSIM_INLINE=1: plain runs with the chain from the seed scale on (the first implementation's sequence)
      static const bool inlineOnly = getenv("XMSIM_INLINE") && atoi(getenv("XMSIM_INLINE")) != 0;
      // (the product sizes a batch by its longest mate and by whether any read is paired - xm_pass_plan.h, seedScaleOf and BatchPolicy; here every read by its
      // own longest mate and its own mates, with the product's default knobs)
      int longestMate = 0;
      for (int m = 0; m < in.nMates; m++) longestMate = std::max(longestMate, (int)in.mateLen[m]);
      const BatchFacts facts{longestMate, in.nMates > 1, 1, 0};
      const BatchPolicy pol = makePolicy(facts, readPassKnobs(facts, knobDefault));
      static const int lightLevel = getenv("XMSIM_LIGHT_LEVEL") ? atoi(getenv("XMSIM_LIGHT_LEVEL")) : 0;
      // light pass -> gapped pass hand-over (runReadRetaining / runReadResumed): the read's region outlives the light "lane"; the gapped pass
      // runs on another context object and another temporaries buffer, as it does on another lane of the GPU
      static const bool handOver = !(getenv("XMSIM_NO_HANDOVER") && atoi(getenv("XMSIM_NO_HANDOVER")) != 0);
      PassState st = firstPass(pol);
      if (!handOver || inlineOnly) st.hoMode = 0;  // (XM_HANDOVER=0)
      if (inlineOnly) st.heavy = true;
      const size_t regionBytes = pol.regionBytes;
      std::vector<double> regionBuf(regionBytes / 8 + 2);
      uint8_t* region = (uint8_t*)(((uintptr_t)regionBuf.data() + 15) & ~(uintptr_t)15);
      SavedRead* saved = nullptr;
      static ReadCtx cx2;
      std::vector<uint8_t> arena2;
      while (true) {
        const int scale = st.scale;
        size_t bytes = pol.arenaUnit * (size_t)scale;
        ReadResult rr;
        DevCounters before = dc;
        // the rejection filter in front of PathAligner (xm_bound.h): the product turns it on for the gapped passes of batches of long reads (planLaunch, boundFilter)
        static const bool boundFilterOn = !(getenv("XMSIM_BOUND_FILTER") && atoi(getenv("XMSIM_BOUND_FILTER")) == 0);
        xmSetBoundFilter(boundFilterOn && pol.filterAllowed(st.heavy, scale) ? 1 : 0);  // (one read per "wave": never more than XM_BOUND_REGIONS)
        if (st.hoMode == 2 && saved) {
          arena2.assign(bytes + chainExtraTmpBytes(scale) + 64, 0xAB);
          uint8_t* a2 = (uint8_t*)(((uintptr_t)arena2.data() + 15) & ~(uintptr_t)15);
          runReadResumed(cx2, saved, &idx->view, scale, a2, pol.gappedTmpBytes(bytes), &dc, rr);
          cx.status = cx2.status;
          cx.persist = cx2.persist; cx.tmp = cx2.tmp;  // (for the overflow trace)
        } else {
          arena.resize(bytes + chainExtraTmpBytes(scale) + 64);
          uint8_t* a = (uint8_t*)(((uintptr_t)arena.data() + 15) & ~(uintptr_t)15);
          if (st.hoMode == 1) {
            runReadRetaining(cx, &idx->view, params, in, scale, region, regionBytes, a, pol.lightTmpUnit * (size_t)scale, &dc, rr, lightLevel);
            st.nRegions = 1; st.regionsTotal = regionBytes;  // (the pool of the light pass: this read's region)
            if (cx.status == XM_ST_NEED_HEAVY) {
              SavedRead* sv = savedReadOf(region, regionBytes);
              saved = sv->valid ? sv : nullptr;
              std::vector<uint8_t>().swap(arena);  // the light lane's temporaries are gone (a stale pointer into them would be caught by the sanitizer run)
            }
          } else if (st.hoMode == 2) {
            // gapped pass, read without saved state (stopped where it cannot be resumed): seeded again in a region of light-pass size
            runReadRetaining(cx, &idx->view, params, in, pol.seedScale, region, regionBytes, a, pol.gappedTmpBytes(bytes), &dc, rr, 2, scale);
          } else {
            runRead(cx, &idx->view, params, in, scale, a, bytes, &dc, rr, st.heavy ? 2 : lightLevel);
          }
        }
        saved = st.hoMode == 1 ? saved : nullptr;  // (consumed, or not wanted any more)
        // what the read's lane files it as (publishRead): the list of the gapped pass, or of the rerun at a larger scale
        PassCtl ctl;
        memset(&ctl, 0, sizeof(ctl));
        if (cx.status == XM_ST_NEED_HEAVY && !st.heavy) ctl.nHeavy = 1;
        else if (cx.status == XM_ST_OVERFLOW) ctl.nScale[st.ts] = 1;
        else if (cx.status != XM_OK) throw std::runtime_error("Failed to align query " + std::to_string(q) + " (status " + std::to_string(cx.status) + ")");
        if (cx.status == XM_ST_OVERFLOW && getenv("XMSIM_TRACE_OVERFLOW")) fprintf(stderr, "[xmsim] query %lld overflow at %s scale %d: persist %zu of %zu%s, tmp %zu of %zu%s\n", (long long)q, st.heavy ? "gapped / rerun" : "light", scale, cx.persist.used, cx.persist.size, cx.persist.overflow ? " (overflow)" : "", cx.tmp.used, cx.tmp.size, cx.tmp.overflow ? " (overflow)" : "");
        const NextPass np = nextPass(pol, st, ctl);
        if (np.kind != PassKind::Done) {
          dc = before;  // work of a read that is rerun by a later pass is counted there
          if (np.kind == PassKind::ScaleRerun) { rerun++; saved = nullptr; }
          continue;
        }
        int64_t ni, nd;
        resultSize(rr, ni, nd);
        res->int_off[q] = (int64_t)ints.size(); res->dbl_off[q] = (int64_t)dbls.size();
        ints.resize(ints.size() + (size_t)ni); dbls.resize(dbls.size() + (size_t)nd);
        OutWriter w;
        w.ints = ints.data() + res->int_off[q]; w.dbls = dbls.data() + res->dbl_off[q]; w.ni = 0; w.nd = 0;
        resultWrite(rr, w, &dc);
        break;
      }
    }
    res->int_off[nq] = (int64_t)ints.size(); res->dbl_off[nq] = (int64_t)dbls.size();
    res->num_ints = (int64_t)ints.size(); res->num_dbls = (int64_t)dbls.size();
    res->ints = (int32_t*)malloc(sizeof(int32_t) * (ints.size() + 1));
    res->dbls = (double*)malloc(sizeof(double) * (dbls.size() + 1));
    if (!ints.empty()) memcpy(res->ints, ints.data(), ints.size() * sizeof(int32_t));
    if (!dbls.empty()) memcpy(res->dbls, dbls.data(), dbls.size() * sizeof(double));
    countersToResult(dc, res);
    res->counters[11] = rerun;
    res->extra[3] = (dc.boundChecks | dc.boundPieceChecks) > 0 ? 1 : 0;
    *out = res;
    return 0;
  } catch (std::exception& e) { g_err = e.what(); return 1; }
}

// the rejection filter of xm_bound.h alone on one problem (what xm_test_bound runs on the GPU); out3: taken, rejected, cells
int xmsim_test_bound(const xm_params* p, const uint8_t* query, int queryLength, int queryRc, int startA, int endA, const uint8_t* reference, int referenceLength, int startB, int endB,
                     int predictedBestOffset, int64_t* out3) {
  const BoundProblem bp = boundTestProblem(*p, query, queryLength, queryRc, startA, endA, reference, referenceLength, startB, endB, predictedBestOffset);
  bool taken = false;
  unsigned long long cells = 0;
  static thread_local std::vector<uint8_t> arena(64 * 1024 + 64);
  Arena tmp;
  tmp.init((void*)(((uintptr_t)arena.data() + 15) & ~(uintptr_t)15), 64 * 1024);
  const bool rejected = boundRejects(bp, false, tmp, taken, cells);
  out3[0] = taken ? 1 : 0; out3[1] = rejected ? 1 : 0; out3[2] = (int64_t)cells;
  return 0;
}

// 0: lane-per-read sequence only, 1: the wave form's light tier first, 2: light then heavy tier first (the product's sequence)
void xmsim_set_wave_mode(int mode) { g_waveMode = mode; }
// how the wave form left the reads of all calls so far, by status (0 = finished there)
void xmsim_wave_status_counts(long long* out, int reset) { for (int i = 0; i < 16; i++) { out[i] = g_waveStatus[i]; if (reset) g_waveStatus[i] = 0; } }
void xmsim_wave_why_counts(long long* out) { for (int i = 0; i < 64; i++) out[i] = g_waveWhy[i]; }

#if defined(XM_ARENA_TRACE)
// The light pass's footprint in a lane's scratch, structure by structure: every read of the batch through runReadRetaining at the light pass's
// settings (scale 1, region + 48 KB of temporaries, heavyAllowed 0) over memory filled with a pattern; per allocation of the two arenas (in
// allocation order: the order is the same for every single-end read without ambiguity codes) the bytes that no longer hold the pattern.
// out[3 * i + 0] = arena (0 region, 1 temporaries), [1] = capacity in bytes, [2] = bytes written, summed over the reads; returns the number of rows.
int64_t xmsim_light_footprint(void* idxp, const xm_params* p, const xm_query_batch* b, int64_t* out, int64_t capRows, int64_t* readsDone) {
  SimIndex* idx = (SimIndex*)idxp;
  const Params params = paramsFromC(*p);
  {
    int maxLen = 1;
    for (int64_t q = 0; q < b->num_queries; q++) for (int m = 0; m < b->mate_count[q]; m++) if (b->mate_length[q * 2 + m] > maxLen) maxLen = b->mate_length[q * 2 + m];
    if (maxLen > idx->host.maxHashedLength) { idx->host.ensureLength(maxLen); idx->refresh(); }
  }
  const BatchFacts facts{1, false, 1, 0};  // (single reads of up to 320 bases)
  const BatchPolicy pol = makePolicy(facts, readPassKnobs(facts, knobDefault));
  const size_t regionBytes = pol.regionBytes, tmpBytes = pol.lightTmpUnit;
  std::vector<uint8_t> region(regionBytes + 64), tmp(tmpBytes + 64);
  uint8_t* rg = (uint8_t*)(((uintptr_t)region.data() + 15) & ~(uintptr_t)15);
  uint8_t* tp = (uint8_t*)(((uintptr_t)tmp.data() + 15) & ~(uintptr_t)15);
  static ReadCtx cx;
  int64_t rows = 0;
  *readsDone = 0;
  for (int64_t q = 0; q < b->num_queries; q++) {
    if (b->mate_count[q] != 1) continue;
    ReadIn in;
    in.nMates = 1;
    for (int m = 0; m < 2; m++) { in.mate[m] = b->codes + b->mate_offset[q * 2 + m]; in.mateLen[m] = m < 1 ? b->mate_length[q * 2 + m] : 0; }
    in.expectedInner = 0.0; in.deviation = 1.0;
    memset(rg, 0xCD, regionBytes); memset(tp, 0xCD, tmpBytes);
    g_allocs.clear();
    g_traceOn = true;
    DevCounters dc; memset(&dc, 0, sizeof(dc));
    ReadResult rr;
    runReadRetaining(cx, &idx->view, params, in, 1, rg, regionBytes, tp, tmpBytes, &dc, rr, 0);
    g_traceOn = false;
    if ((int64_t)g_allocs.size() > capRows) return -1;
    if ((int64_t)g_allocs.size() > rows) { for (int64_t i = rows; i < (int64_t)g_allocs.size(); i++) { out[3 * i] = 0; out[3 * i + 1] = 0; out[3 * i + 2] = 0; } rows = (int64_t)g_allocs.size(); }
    for (size_t i = 0; i < g_allocs.size(); i++) {
      const ArenaAlloc& a = g_allocs[i];
      const uint8_t* base = (const uint8_t*)a.base;
      const int arena = base == rg ? 0 : 1;
      int64_t dirty = 0;
      for (size_t k = 0; k < a.bytes; k++) if (base[a.offset + k] != 0xCD) dirty++;
      out[3 * i] = arena; if ((int64_t)a.bytes > out[3 * i + 1]) out[3 * i + 1] = (int64_t)a.bytes; out[3 * i + 2] += dirty;
    }
    (*readsDone)++;
  }
  return rows;
}
#endif


void xmsim_result_free(xm_result* r) {
  if (!r) return;
  free(r->ints); free(r->dbls); free(r->int_off); free(r->dbl_off); free(r);
}

int xmsim_table_info(void* idxp, int L, int32_t* capacity, int32_t* maxCount, int64_t* numStored) {
  SimIndex* idx = (SimIndex*)idxp;
  if (L < 0 || L > idx->host.maxHashedLength) return 1;
  const Table& t = idx->host.tables[(size_t)L];
  *capacity = t.capacity; *maxCount = t.maxCount;
  *numStored = (int64_t)(idx->host.bucketOff[(size_t)(t.offBase + t.capacity)] & ~XM_OVERFULL);
  return 0;
}
int xmsim_table_dump(void* idxp, int L, int32_t* counts, int64_t* positionsOut) {
  SimIndex* idx = (SimIndex*)idxp;
  const HostIndex& h = idx->host;
  const Table& t = h.tables[(size_t)L];
  int64_t w = 0;
  for (int k = 0; k < t.capacity; k++) {
    uint32_t o0 = h.bucketOff[(size_t)(t.offBase + k)], o1 = h.bucketOff[(size_t)(t.offBase + k + 1)];
    if (o0 & XM_OVERFULL) { counts[k] = -1; continue; }
    int c = (int)((o1 & ~XM_OVERFULL) - (o0 & ~XM_OVERFULL));
    counts[k] = c;
    for (int j = 0; j < c; j++) positionsOut[w++] = (int64_t)h.positions[(size_t)(t.posBase + (o0 & ~XM_OVERFULL) + j)];
  }
  return 0;
}
int xmsim_index_info(void* idxp, int32_t* minInteresting, int32_t* maxHashed) {
  SimIndex* idx = (SimIndex*)idxp;
  *minInteresting = idx->host.minInterestingSize; *maxHashed = idx->host.maxHashedLength;
  return 0;
}
int xmsim_ensure_length(void* idxp, int length) {
  SimIndex* idx = (SimIndex*)idxp;
  try { idx->host.ensureLength(length); idx->refresh(); return 0; } catch (std::exception& e) { g_err = e.what(); return 1; }
}
int64_t xmsim_dup_keys(void* idxp, int contig, int32_t* out, int64_t cap) {
  SimIndex* idx = (SimIndex*)idxp;
  const HostIndex& h = idx->host;
  int64_t a = h.dupKeyStart[(size_t)contig], bb = h.dupKeyStart[(size_t)contig + 1];
  for (int64_t i = a; i < bb && i - a < cap; i++) out[i - a] = h.dupKeys[(size_t)i];
  return bb - a;
}

// T/MultiHashBlock_Test.java:84-133 through the product's reference-side multi blocks (HostIndex::nextLevelMulti, the code that hashes the windows
// around ambiguous bases): the possibilities of the blocks that start at 0 and end at the end of `ambiguous` (4-bit codes) must hold the block the
// plain rule makes of `text`.  0 = they do; 1 = they do not; 2 = `text` has no single block over its whole length.
int xmsim_kat_multi_contains(const uint8_t* text, const uint8_t* ambiguous, int len) {
  // the plain pyramid of `text`: the block at 0 that ends at len, if a level has one
  bool have = false;
  HBlock want{};
  {
    std::vector<HBlock> cur((size_t)len), next;
    for (int i = 0; i < len; i++) cur[(size_t)i] = HostIndex::hblock0(text[i], i);
    while (!cur.empty()) {
      if (cur[0].start == 0 && cur[0].len == len) { have = true; want = cur[0]; }
      next.clear();
      for (size_t i = 0; i + 1 < cur.size(); i++) if (shouldMergeBlocks(cur[i], cur[i + 1])) next.push_back(mergeBlocks(cur[i], cur[i + 1]));
      cur.swap(next);
    }
  }
  if (!have) return 2;
  std::vector<HostIndex::HEntry> cur((size_t)len);
  for (int i = 0; i < len; i++) {
    HostIndex::HEntry& e = cur[(size_t)i];
    const uint8_t code = ambiguous[i];
    if (bpIsAmbiguous(code)) {
      e.multi = true;
      for (int bit = 0; bit < 4; bit++) if (code & (1 << bit)) e.poss.push_back(HostIndex::HPoss{HostIndex::hblock0((uint8_t)(1 << bit), i), true, HostIndex::HCond(1, std::make_pair((int32_t)i, (uint8_t)(1 << bit)))});
    } else e.single = HostIndex::hblock0(code, i);
  }
  while (!cur.empty()) {
    for (const HostIndex::HEntry& e : cur) {
      if (e.start() != 0) continue;
      for (const HostIndex::HPoss& p : HostIndex::possibilitiesOf(e))
        if (p.hasBlock && p.block.start == 0 && p.block.len == len && p.block.fwd == want.fwd) return 0;
    }
    std::vector<HostIndex::HEntry> nx = HostIndex::nextLevelMulti(cur);
    cur.swap(nx);
  }
  return 1;
}

// T/SequenceDatabase_Test.java:16-42,118-132 through the product's position codec: HostIndex::encodePosition / decode on the host and decodePosition
// (xm_seed.h, what the kernels run) over the same cumulative starts, for numSequences contigs of sequenceLength - i bases and their reverse
// complements; positions 0, 100, length - 100, length - 1.  0 = every round trip holds.
int xmsim_kat_position_codec(int numSequences, int sequenceLength) {
  HostIndex h;
  int64_t off = 0;
  for (int i = 0; i < numSequences; i++) {
    const int64_t len = (int64_t)sequenceLength - i;
    h.contigStart.push_back(off); h.contigLen.push_back((int32_t)len);
    h.seqCumStart.push_back(2 * off); h.seqCumStart.push_back(2 * off + len);
    off += len;
  }
  h.seqCumStart.push_back(2 * off);
  h.totalForwardSize = off;
  IndexView v;
  memset(&v, 0, sizeof(v));
  v.numContigs = numSequences; v.seqCumStart = h.seqCumStart.data(); v.contigLen = h.contigLen.data(); v.contigStart = h.contigStart.data();
  for (int c = 0; c < numSequences; c++)
    for (int rc = 0; rc < 2; rc++) {
      const int n = h.contigLen[(size_t)c];
      const int positions[4] = {0, 100, n - 100, n - 1};
      for (int k = 0; k < 4; k++) {
        const int position = positions[k];
        if (position < 0 || position >= n) continue;
        const int64_t enc = h.encodePosition(c, rc != 0, position);
        int dc = -1, ds = -1; bool drc = false;
        h.decode(enc, dc, drc, ds);
        if (dc != c || drc != (rc != 0) || ds != position) return 1;
        const RefPos p = decodePosition(v, enc);
        if (p.contig != c || (p.rc != 0) != (rc != 0) || p.start != position) return 2;
      }
    }
  return 0;
}

// read-side pyramid dump in the layout of oracle xmo_pyramid_dump (14 ints per block)
int64_t xmsim_pyramid_dump(const uint8_t* codes, int len, int32_t* out, int64_t capRows) {
  std::vector<PBlock> blocks((size_t)len * 64 + 64);
  std::vector<int32_t> ls((size_t)len + 8);
  int32_t status = 0;
  SeqView s;
  s.base = codes; s.len = len; s.rc = 0; s.id = 0;
  Pyramid pyr;
  pyr.init(s, blocks.data(), (int)blocks.size(), ls.data(), len + 4, &status);
  int64_t n = 0;
  for (int level = 0;; level++) {
    if (level > 0) { pyr.ensure(level); if (status) return -1; }
    int cnt = pyr.count(level);
    if (cnt == 0) break;
    for (int i = 0; i < cnt; i++) {
      PBlock h = pyr.blockAt(level, i);
      if (n < capRows) {
        int32_t* o = out + n * 14;
        o[0] = level; o[1] = h.start; o[2] = h.len; o[3] = h.fwd; o[4] = h.rev; o[5] = h.flags; o[6] = h.gapDir; o[7] = h.extraGap;
        QBlock g;
        int st = withGapAndExtension(h, s, g);
        o[8] = st; o[9] = st ? g.start : 0; o[10] = st ? g.len : 0; o[11] = st ? g.used : 0; o[12] = st ? g.fwd : 0; o[13] = st ? g.rev : 0;
      }
      n++;
    }
  }
  return n;
}

// the same with the multi blocks of a read with ambiguous bases, in the layout of the oracle's xmo_pyramid_dump_multi (12 ints per possibility);
// `scale` sizes the pools as compInit does.  -1: a capacity was exceeded (on the GPU: the read runs again with more scratch)
int64_t xmsim_pyramid_dump_multi(const uint8_t* codes, int len, int scale, int32_t* out, int64_t capRows) {
  std::vector<PBlock> blocks((size_t)len * 64 + 64);
  std::vector<int32_t> ls((size_t)len + 8);
  int32_t status = 0;
  SeqView s;
  s.base = codes; s.len = len; s.rc = 0; s.id = 0;
  Pyramid pyr;
  pyr.init(s, blocks.data(), (int)blocks.size(), ls.data(), len + 4, &status);
  MultiStore ms;
  const MultiCaps mc = multiCaps(scale);
  std::vector<Poss> pool((size_t)mc.pool);
  std::vector<CondEnt> conds((size_t)mc.conds), stack((size_t)mc.stack);
  std::vector<MFrame> frames((size_t)mc.frames);
  ms.pool = pool.data(); ms.poolUsed = 0; ms.poolCap = (int)pool.size();
  ms.conds = conds.data(); ms.condUsed = 0; ms.condCap = (int)conds.size();
  ms.stack = stack.data(); ms.stackCap = (int)stack.size();
  ms.frames = frames.data(); ms.framesCap = (int)frames.size();
  bool amb = false;
  for (int i = 0; i < len; i++) if (bpIsAmbiguous(codes[i])) amb = true;
  if (amb) pyr.ms = &ms;
  int64_t n = 0;
  for (int level = 0;; level++) {
    if (level > 0) { pyr.ensure(level); if (status) return -1; }
    int cnt = pyr.count(level);
    if (cnt == 0) break;
    for (int i = 0; i < cnt; i++) {
      const PBlock e = amb ? pyr.entryAt(level, i) : pyr.blockAt(level, i);
      const bool multi = (e.flags & F_MULTI) != 0;
      const int np = multi ? pyr.numPoss(level, e) : 1;
      for (int k = 0; k < np; k++) {
        PossView p;
        pyr.possAt(level, e, k, p);
        if (n < capRows) {
          int32_t* o = out + n * 12;
          o[0] = level; o[1] = e.start; o[2] = e.len; o[3] = multi ? np : 0; o[4] = k; o[5] = p.hasBlock;
          o[6] = p.hasBlock ? p.block.start : 0; o[7] = p.hasBlock ? p.block.len : 0; o[8] = p.hasBlock ? p.block.fwd : 0; o[9] = p.hasBlock ? p.block.rev : 0;
          o[10] = p.hasBlock ? (p.block.flags & 15) : 0;
          uint32_t hash = multi ? (uint32_t)p.condLen : 0u;
          if (multi) for (int t = 0; t < p.condLen; t++) hash = hash * 1000003u + ((p.cond[t] >> 2) * 4u + (p.cond[t] & 3u));
          o[11] = (int32_t)hash;
        }
        n++;
      }
    }
  }
  return n;
}

// ---- the product's pass planner (mapper_amd/csrc/xm_pass_plan.h) for tests/test_pass_plan.py.  facts: longest mate, any paired, contexts on the GPU, scratch limit
// of the context in bytes (0: none).  The knobs are read from the environment as an align call reads them.  state (11): heavy, hoMode, scale, overflowScale,
// orderedList, ts, to, tc, confRounds, nRegions, regionsTotal.  Non-zero: failed, xmsim_last_error() says why.
static BatchPolicy simPolicy(const int64_t* f) {
  const BatchFacts facts{(int)f[0], f[1] != 0, (int)f[2], (long long)f[3]};
  return makePolicy(facts, readPassKnobs(facts));
}
static PassState simState(const int64_t* s) { return PassState{s[0] != 0, (int)s[1], (int)s[2], (int)s[3], s[4] != 0, (int)s[5], (int)s[6], (int)s[7], (int)s[8], (long long)s[9], (size_t)s[10]}; }
static void simStateOut(const PassState& st, int64_t* s) {
  s[0] = st.heavy; s[1] = st.hoMode; s[2] = st.scale; s[3] = st.overflowScale; s[4] = st.orderedList; s[5] = st.ts; s[6] = st.to; s[7] = st.tc; s[8] = st.confRounds;
  s[9] = st.nRegions; s[10] = (int64_t)st.regionsTotal;
}
// policy (16): seedScale, gappedScale, longReads, arenaUnit, lightTmpUnit, regionBytes, scratchWanted, boundFilterOn, searchPoolOn, heavyHint, lightWaves, fullWaves,
// lightLpw, fullLpw, gappedTmpBytes(arena of the gapped scale), handOver; state: the first pass's
int xmsim_pass_policy(const int64_t* facts, int64_t* policy, int64_t* state) {
  try {
    const BatchPolicy pol = simPolicy(facts);
    const int64_t v[16] = {pol.seedScale, pol.gappedScale, pol.longReads, (int64_t)pol.arenaUnit, (int64_t)pol.lightTmpUnit, (int64_t)pol.regionBytes, (int64_t)pol.scratchWanted, pol.boundFilterOn,
                           pol.searchPoolOn, pol.k.heavyHint, pol.k.lightWaves, pol.k.fullWaves, pol.k.lightLpw, pol.k.fullLpw, (int64_t)pol.gappedTmpBytes(pol.arenaUnit * (size_t)pol.gappedScale), pol.k.handOver};
    for (int i = 0; i < 16; i++) policy[i] = v[i];
    simStateOut(firstPass(pol), state);
    return 0;
  } catch (std::exception& e) { g_err = e.what(); return 1; }
}
// plan (16): arenaBytes, lpw, nWaves, grid, block, lanes, nRegions, regionsTotal, scratchBytes, gappedReserve, pairLanes, boundFilter, boundFilterArg, firstStride, firstItem, poolBuffers;
// plan[16] = taperUnit
int xmsim_plan_launch(const int64_t* facts, const int64_t* state, int64_t nTodo, int64_t nq, int numCUs, uint64_t budget, uint64_t scratchHeld, int64_t* plan) {
  try {
    const LaunchPlan pl = planLaunch(simPolicy(facts), simState(state), nTodo, nq, numCUs, budget, (size_t)scratchHeld);
    const int64_t v[17] = {(int64_t)pl.arenaBytes, pl.lpw, pl.nWaves, pl.grid, pl.block, pl.lanes, pl.nRegions, (int64_t)pl.regionsTotal, (int64_t)pl.scratchBytes, (int64_t)pl.gappedReserve, pl.pairLanes,
                           pl.boundFilter, pl.boundFilterArg, pl.firstStride, (int64_t)pl.firstItem, pl.poolBuffers, pl.taperUnit};
    for (int i = 0; i < 17; i++) plan[i] = v[i];
    return 0;
  } catch (std::exception& e) { g_err = e.what(); return 1; }
}
// ctl (9): nHeavy, nHeavyLate, nScale[2], nOut[2], errQuery, nConf[2]; state is updated; next (4): kind (0 done, 1 result-arena rerun, 2 gapped, 3 confidence rerun,
// 4 scale rerun), nTodo, list, clear
int xmsim_next_pass(const int64_t* facts, int64_t* state, const uint64_t* ctl, int64_t* next) {
  try {
    PassState st = simState(state);
    const PassCtl c{ctl[0], ctl[1], {ctl[2], ctl[3]}, {ctl[4], ctl[5]}, ctl[6], {ctl[7], ctl[8]}};
    const NextPass np = nextPass(simPolicy(facts), st, c);
    simStateOut(st, state);
    next[0] = (int64_t)np.kind; next[1] = np.nTodo; next[2] = np.list; next[3] = np.clear;
    return 0;
  } catch (std::exception& e) { g_err = e.what(); return 1; }
}
// the result arenas' sizes (elements): what a call of nq queries with `hits` replayed elements starts with (doubles: the doubles' arena), what a full one grows to
uint64_t xmsim_first_arena_size(int64_t nq, uint64_t hits, int doubles) { return (uint64_t)firstArenaSize(nq, hits, doubles != 0); }
uint64_t xmsim_grown_arena_size(uint64_t cap, uint64_t cursor) { return (uint64_t)grownArenaSize(cap, cursor); }

// ---- the index-build planner (mapper_amd/csrc/xm_index_plan.h, what the host builder and the GPU builder share) for tests/test_index_plan.py
// out (2): capacity, maxCount
void xmsim_table_shape(int64_t estimatedCapacity, int L, int maxNumShortMatches, int64_t* out) {
  const TableShape t = tableShape(estimatedCapacity, L, maxNumShortMatches);
  out[0] = t.capacity; out[1] = t.maxCount;
}
// hist [maxLen + 1]; out (3 per group): gLo, gHi, nRecs (the first capGroups of them) -> how many groups
int64_t xmsim_plan_groups(const uint64_t* hist, int minLen, int maxLen, uint64_t budgetRecs, int64_t* out, int64_t capGroups) {
  const std::vector<TableGroup> groups = planGroups(std::vector<unsigned long long>(hist, hist + maxLen + 1), minLen, maxLen, budgetRecs);
  for (size_t i = 0; i < groups.size() && (int64_t)i < capGroups; i++) { out[3 * i] = groups[i].gLo; out[3 * i + 1] = groups[i].gHi; out[3 * i + 2] = (int64_t)groups[i].nRecs; }
  return (int64_t)groups.size();
}
// hist, capacity, maxCount [gHi + 1] (the planned shapes); out (3 per table of [gLo, gHi]): bucketBase, capacity, maxCount -> nEntries
int64_t xmsim_layout_group(const uint64_t* hist, const int32_t* capacity, const int32_t* maxCount, int gLo, int gHi, int64_t* out) {
  std::vector<TableShape> shapes((size_t)gHi + 1);
  for (int L = 0; L <= gHi; L++) shapes[(size_t)L] = TableShape{capacity[L], maxCount[L]};
  const GroupLayout lay = layoutGroup(TableGroup{gLo, gHi, 0}, std::vector<unsigned long long>(hist, hist + gHi + 1), shapes);
  for (size_t k = 0; k < lay.tables.size(); k++) { out[3 * k] = (int64_t)lay.tables[k].bucketBase; out[3 * k + 1] = lay.tables[k].capacity; out[3 * k + 2] = lay.tables[k].maxCount; }
  return (int64_t)lay.nEntries;
}
// out (2): posBits, tableBits
void xmsim_sort_key_bits(uint64_t lastCumStart, int ambiguous, int nTables, int64_t* out) {
  const SortKeyBits b = sortKeyBits(lastCumStart, ambiguous != 0, nTables);
  out[0] = b.posBits; out[1] = b.tableBits;
}

// ---- the host's confidence table (mapper_amd/csrc/xm_conf_table.h) for tests/test_conf_table.py: a ConfTable driven as a context drives it, and read with the
// kernels' own lookup (confLookup, xm_defs.h)
void* xmsim_conf_new(void) { return new ConfTable(); }
void xmsim_conf_free(void* t) { delete (ConfTable*)t; }
void xmsim_conf_prepare(void* t, const xm_params* p, const int32_t* lens, int64_t nLens, double granularity, int64_t totalSize, int64_t seedBudget) {
  ((ConfTable*)t)->prepare(paramsFromC(*p), std::vector<int32_t>(lens, lens + nLens), granularity, totalSize, seedBudget);
}
// added[i] = what insert returned for key i; -> how many were added
int64_t xmsim_conf_insert(void* t, int64_t n, const double* penalties, const int32_t* lens, uint8_t* added) {
  int64_t k = 0;
  for (int64_t i = 0; i < n; i++) { added[i] = ((ConfTable*)t)->insert(penalties[i], lens[i]) ? 1 : 0; k += added[i]; }
  return k;
}
// found[i], values[i] = confLookup over the table's slots; -> how many were found
int64_t xmsim_conf_lookup(void* t, int64_t n, const double* penalties, const int32_t* lens, uint8_t* found, double* values) {
  const ConfTable& c = *(ConfTable*)t;
  int64_t k = 0;
  for (int64_t i = 0; i < n; i++) { values[i] = 0; found[i] = confLookup(c.data(), c.mask(), penalties[i], lens[i], values[i]) ? 1 : 0; k += found[i]; }
  return k;
}
// out (3): slots, entries, dirty
void xmsim_conf_state(void* t, int64_t* out) { const ConfTable& c = *(ConfTable*)t; out[0] = (int64_t)c.size(); out[1] = (int64_t)c.used(); out[2] = c.dirty() ? 1 : 0; }
void xmsim_conf_mark_uploaded(void* t) { ((ConfTable*)t)->markUploaded(); }
// every entry, in slot order -> their number (cap: room in the arrays)
int64_t xmsim_conf_dump(void* t, int64_t cap, double* penalties, int32_t* lens, double* values) {
  const ConfTable& c = *(ConfTable*)t;
  int64_t k = 0;
  for (size_t i = 0; i < c.size(); i++) {
    const ConfEntry& e = c.data()[i];
    if (!e.used) continue;
    if (k < cap) { memcpy(&penalties[k], &e.penaltyBits, 8); lens[k] = e.queryLength; values[k] = e.totalLengthForHighConfidence; }
    k++;
  }
  return k;
}
void xmsim_conf_values(int64_t n, const double* penalties, const int32_t* lens, double maxPenaltySpan, double mutationPenalty, double granularity, int64_t totalSize, double* values) {
  for (int64_t i = 0; i < n; i++) values[i] = confidenceLengthOnHost(penalties[i], lens[i], maxPenaltySpan, mutationPenalty, granularity, totalSize);
}

}  // extern "C"
