// The plan of an align call (xm_capi.hip, alignResidentLocked), as plain host C++: the knobs, the policy of a batch, the shape of a launch of the
// lane-per-read passes and the sequence of the passes.  No HIP, no allocation, and the arithmetic reads no environment: the product calls it between
// its launches, the host simulation (tests/hostsim) takes its sizes from it, and tests/test_pass_plan.py checks it without a GPU.
#pragma once
#include "../../include/xmapper_hip.h"
#include "xm_kernel_common.h"
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace xm {

inline long long envInt(const char* name, long long dflt) {
  const char* v = getenv(name);
  return (v && *v) ? atoll(v) : dflt;
}
// experiment knobs are validated: a value outside [lo, hi] (or not a power of two where the capacities need one) is an error, not a silent corruption
inline long long envKnob(const char* name, long long dflt, long long lo, long long hi, bool pow2 = false) {
  const long long v = envInt(name, dflt);
  if (v < lo || v > hi || (pow2 && (v & (v - 1)) != 0))
    throw std::runtime_error(std::string(name) + "=" + std::to_string(v) + " is not valid: expected " + (pow2 ? "a power of two in " : "a value in ") + std::to_string(lo) + ".." + std::to_string(hi));
  return v;
}
// where the knobs come from: envKnob in the product, knobDefault in the host simulation (which has its own XMSIM_* switches and runs the product's defaults)
typedef long long (*KnobReader)(const char* name, long long dflt, long long lo, long long hi, bool pow2);
inline long long knobDefault(const char*, long long dflt, long long, long long, bool) { return dflt; }

inline Params paramsFromC(const xm_params& p) {
  Params params;
  params.MutationPenalty = p.MutationPenalty; params.InsertionStart_Penalty = p.InsertionStart_Penalty; params.InsertionExtension_Penalty = p.InsertionExtension_Penalty;
  params.DeletionStart_Penalty = p.DeletionStart_Penalty; params.DeletionExtension_Penalty = p.DeletionExtension_Penalty; params.MaxErrorRate = p.MaxErrorRate;
  params.UnalignedPenalty = p.UnalignedPenalty; params.AmbiguityPenalty = p.AmbiguityPenalty; params.Max_PenaltySpan = p.Max_PenaltySpan;
  params.MaxNumMatches = p.MaxNumMatches; params.StartingInsertionStartFree = 0;
  return params;
}
// (counters[11..15], extra[3], extra[7] and prof are the caller's: reruns, kernel times, whether the filter ran, copies)
inline void countersToResult(const DevCounters& dc, xm_result* res) {
  res->counters[0] = (int64_t)dc.reads; res->counters[1] = (int64_t)dc.headerProbes; res->counters[2] = (int64_t)dc.bucketFetches; res->counters[3] = (int64_t)dc.hitsFetched;
  res->counters[4] = (int64_t)dc.candidatesExtended; res->counters[5] = (int64_t)dc.pathAlignerCalls; res->counters[6] = (int64_t)dc.pathAlignerNodes;
  res->counters[7] = (int64_t)dc.quickAccepts; res->counters[8] = (int64_t)dc.alignmentsOut; res->counters[9] = (int64_t)dc.refWindowBytes; res->counters[10] = (int64_t)dc.readBytes;
  res->extra[0] = (int64_t)dc.boundChecks; res->extra[1] = (int64_t)dc.boundRejects; res->extra[2] = (int64_t)dc.boundCells; res->extra[4] = (int64_t)dc.boundPieceChecks; res->extra[5] = (int64_t)dc.boundPieceRejects;
}

// The two result arenas of a context (ResultStage, xm_result_stage.h), in elements.  What a call of nq queries starts with: room for a typical batch
// (40 ints and 12 doubles per query) plus `hits`, the elements of the slices a run-wide memory replays into the arena before the first pass.  What an
// arena that a pass found full (cursor: what the pass asked for, beyond cap) grows to before the rerun: four times as much, and at least twice the need.
inline size_t firstArenaSize(long long nq, unsigned long long hits, bool doubles) { return (size_t)nq * (doubles ? 12 : 40) + 4096 + (size_t)hits; }
inline unsigned long long grownArenaSize(unsigned long long cap, unsigned long long cursor) { return std::max(cap * 4 + 65536, cursor * 2); }

constexpr long long XM_ARENA_KB_DEFAULT = 288;  // scratch of a lane at scale 1

// what the plan of a call depends on besides the knobs
struct BatchFacts {
  int longestMate;                // of the batch
  bool anyPaired;
  int gpuContexts;                // contexts that exist on the GPU (DeviceTables::contexts)
  long long contextScratchBytes;  // xm_context_set_scratch (0: XM_SCRATCH_GIB / the default)
};

// the scratch capacities are sized for ~150-300 bp mates at scale 1; batches of longer reads start at a larger scale instead of
// sending every read through a pass that can only overflow
inline int seedScaleOf(int longestMate) { return longestMate <= 320 ? 1 : (longestMate <= 1280 ? 4 : 16); }

// Every XM_* variable the lane-per-read passes of an align call read (the wave-per-read driver reads its own: XM_WAVE_TIERS, XM_WAVE_FETCH,
// XM_WAVE_CHAIN_FETCH, XM_WAVE_INLINE_SEARCH), filled once per call by readPassKnobs: tests set them between the calls of one process, and the
// defaults depend on the batch.  All of them are experiment knobs.
struct PassKnobs {
  long long gappedScale;    // XM_GAPPED_SCALE (batches that seed at scale 1) or the seed scale x XM_GAPPED_FACTOR
  long long arenaKb;        // XM_ARENA_KB: scratch of a lane at scale 1 (the capacities do not follow it, a smaller arena only overflows earlier)
  long long scratchGib;     // XM_SCRATCH_GIB: scratch limit of a context without one of its own
  long long lightWaves, fullWaves;  // XM_LIGHT_WAVES, XM_FULL_WAVES: wave slots a launch is sized for, in waves per SIMD
  long long fullLpw, lightLpw;      // XM_FULL_LPW, XM_LIGHT_LPW: reads per wave
  long long lightLevel;     // XM_LIGHT_LEVEL: what the light pass still does itself (Caps::heavyAllowed)
  long long heavyHint;      // XM_HEAVY_HINT: straight-alignment penalty x 8 from which a read is put first in the gapped pass and dealt out evenly (0: no order)
  long long taperPct;       // XM_TAPER_PCT: lane l of a gapped-pass wave stops taking reads when fewer than l * waves * pct/100 are left
  bool pairLanes;           // XM_PAIR_LANES: two lanes per read in the gapped passes
  bool groupLanes;          // XM_GROUP_LANES: eight in the passes that run the rejection filter
  bool boundFilter;         // XM_BOUND_FILTER (0: off, for comparison)
  bool groupSweep;          // XM_GROUP_SWEEP
  bool searchPool;          // XM_SEARCH_POOL
  long long gappedTmpPct;   // XM_GAPPED_TMP_PCT: temporaries of a gapped-pass lane, percent of 7/12 of the arena of that scale
  long long lightTmpKb;     // XM_LIGHT_TMP_KB
  long long regionKb;       // XM_REGION_KB
  bool handOver;            // XM_HANDOVER
  bool waveForm;            // XM_WAVE: the wave-per-read form first (mates of up to 256 bases)
  bool tracePasses;         // XM_TRACE_PASSES
  bool profGappedOnly;      // XM_PROF_GAPPED_ONLY (XM_PROFILE builds: the in-kernel timers of the gapped pass alone)
};

inline PassKnobs readPassKnobs(const BatchFacts& f, KnobReader knob = envKnob) {
  auto flag = [&](const char* name, long long dflt) { return knob(name, dflt, LLONG_MIN, LLONG_MAX, false) != 0; };  // (any integer: non-zero is on)
  PassKnobs k;
  const int seedScale = seedScaleOf(f.longestMate);
  k.gappedScale = seedScale < 4 ? knob("XM_GAPPED_SCALE", 4, 1, 64, true) : seedScale * knob("XM_GAPPED_FACTOR", 4, 1, 64, true);
  k.arenaKb = knob("XM_ARENA_KB", XM_ARENA_KB_DEFAULT, 64, 16384, false);
  k.scratchGib = f.contextScratchBytes > 0 ? 0 : knob("XM_SCRATCH_GIB", 200, 1, 280, false);
  // wave slots a launch is sized for (in waves per SIMD): alone on the GPU a context fills it (4 are resident at 128 registers; the light pass asks
  // for twice that, the second half starts as the first drains).  Contexts that share the GPU (xm_context_new) must leave each other room: a
  // persistent launch that holds every slot keeps the next context's launch waiting until its own tail, and the contexts then run one after the
  // other instead of side by side.  Together the contexts of a GPU ask for 12 waves per SIMD worth of light lanes and 6 of gapped lanes: two contexts 6 / 3
  // each (round 3), three 4 / 2 - 14.1-14.3 M reads/s against 13.1-13.2 with two, once the runtime has hardware queues for three contexts' streams
  // (GPU_MAX_HW_QUEUES, mapper_amd/_capi.py); with 6 / 3 each three contexts measured 12.3-12.7, four with 3 / 1 13.5 (profiles/r04/NOTES.md 15)
  // (the contexts that EXIST on the GPU, not the ones aligning at the moment: sizing by activity was tried in round 5 and made the headline bimodal - a context that
  // finds itself alone launches for the whole GPU, the runtime then gives its queue scratch memory for a whole GPU's waves (5.8 KB per lane), and in about half the
  // runs the other contexts' launches then ran one after the other for the rest of the process, 4.6 M reads/s instead of 15.  A process that keeps contexts it does
  // not use should close them.)
  const bool sharedGpu = f.gpuContexts > 1;
  // Batches of long reads (gapped pass beyond scale 4: every read goes through the chain, and its searches - thousands of nodes each, all in HBM mode -
  // are most of its time): the lanes of a wave run their searches one after the other, so 8 reads per wave on twice as many waves instead of 32
  // (1 kb queries: 382 ms -> 265-280 ms per 150 k; 4 to 8 reads per wave and 8 to 16 waves per SIMD worth of lanes measure the same, profiles/r03/NOTES.md 13)
  const bool longReads = k.gappedScale > 4;
  // (long reads: every lane of the light pass holds a region of the arena's size, and every read goes on to the gapped pass, whose lanes are 6.7 MB each:
  // two waves per SIMD worth of light lanes leave the scratch to those)
  k.lightWaves = knob("XM_LIGHT_WAVES", longReads ? 2 : (sharedGpu ? std::max(2, 12 / f.gpuContexts) : 8), 1, 16, false);
  k.fullWaves = knob("XM_FULL_WAVES", longReads ? 8 : (sharedGpu ? std::max(1, 6 / f.gpuContexts) : 4), 1, 16, false);
  k.fullLpw = knob("XM_FULL_LPW", longReads ? 8 : 32, 1, 64, false);
  k.lightLpw = knob("XM_LIGHT_LPW", 64, 1, 64, false);
  k.lightLevel = knob("XM_LIGHT_LEVEL", 0, 0, 2, false);
  // Batches of single reads of up to 320 bases: 8 penalty units - the reads with an indel (they mismatch on one whole side of it), whose searches are
  // the long ones of the pass: started first they do not end it (gapped pass 70.0 / 70.5 -> 65.2 / 64.8 ms per 1 M reads, same box; with 4 units 75 ms;
  // pairs 146 -> 152-154 ms: not for them)
  k.heavyHint = knob("XM_HEAVY_HINT", (f.anyPaired || longReads) ? 0 : 64, 0, 1 << 20, false);
  k.taperPct = knob("XM_TAPER_PCT", 100, 0, 1000, false);
  k.pairLanes = flag("XM_PAIR_LANES", 1);
  k.groupLanes = flag("XM_GROUP_LANES", 1);
  k.boundFilter = flag("XM_BOUND_FILTER", 1);
  k.searchPool = flag("XM_SEARCH_POOL", 1);
  // temporaries of a gapped-pass lane (reads that resume from a saved region): 7/12 of the arena of that scale by default (percent of it)
  // HBM-mode searches take their arrays from a pool of the launch (SearchPool) in batches of short reads (gapped pass at scale <= 4): a lane's
  // temporaries then hold the chain's structures only (matchers 148 KB + piece lists 23 KB + small change at scale 4; default 30 % of 7/12 of
  // the arena = 201 KB).  Batches of long reads run every search in HBM mode: no pool, whole temporaries.
  k.gappedTmpPct = knob("XM_GAPPED_TMP_PCT", (k.searchPool && k.gappedScale <= 4) ? 20 : 100, 5, 100, false);  // (134 KB: matchers 74 KB, piece lists 23 KB, the rest small change)
  // light pass: a lane's temporaries hold the three matchers alignMatch sets aside (37 KB at scale 1; the chain that would fill them does not
  // run there) and the joined text of overlapping mates; a read's region holds its seeding state: 49 KB single-end, 99 KB paired at scale 1
  // (ambiguity codes add up to 18 KB per mate: a pair with them in both mates overflows its region - and the region of the same size a gapped-pass lane seeds reads
  // without saved state in - so it is filed for the pass behind the gapped pass and run from its start at four times the gapped pass's scale, one read per wave.
  // Correct (the ambiguity fuzz equals the oracle) and late: FASTQ pairs with N tails in both mates pay a latency-bound extra pass.  Known, not fixed: knowing it
  // at upload would mean reading every base of the batch on the host.)
  k.lightTmpKb = knob("XM_LIGHT_TMP_KB", 48, 16, 16384, false);
  k.regionKb = knob("XM_REGION_KB", f.anyPaired ? 120 : 72, 32, 16384, false);
  k.handOver = flag("XM_HANDOVER", 1);
  k.waveForm = flag("XM_WAVE", 0);
  k.groupSweep = flag("XM_GROUP_SWEEP", 1);
  k.tracePasses = flag("XM_TRACE_PASSES", 0);
  k.profGappedOnly = flag("XM_PROF_GAPPED_ONLY", 0);
  return k;
}

// What a batch's passes are sized by: the knobs and what follows from them and the batch.
struct BatchPolicy {
  PassKnobs k;
  int gpuContexts;
  int seedScale, gappedScale;  // the light pass's scale (1 / 4 / 16 by the longest mate); the gapped pass's (4 for short reads, else four times the seed scale)
  bool longReads;              // gapped pass beyond scale 4
  size_t arenaUnit, lightTmpUnit;      // bytes at scale 1: a lane's arena; a light-pass lane's temporaries
  size_t regionBytes;                  // a read's region of the hand-over pool: its seeding state + its SavedRead
  unsigned long long scratchWanted;    // scratch limit of the context
  // (batches of long reads only: where reads align, the filter costs what it saves - 2 % of the search nodes of configs[1], 16 % of a repeat-rich reference's
  // sit in searches it rejects, and it would look at every search: profiles/r06/NOTES.md 1)
  bool boundFilterOn;
  bool searchPoolOn;                   // batches of short reads
  // temporaries of a gapped-pass lane whose arena at that scale is `arena` bytes (+ the node arrays of a long-read chain: applyChainCaps)
  size_t gappedTmpBytes(size_t arena) const { return ((size_t)((arena - arenaPersistBytes(arena)) * (size_t)k.gappedTmpPct / 100) & ~(size_t)15) + chainExtraTmpBytes(gappedScale); }
  // the rejection filter in front of PathAligner's searches (xm_bound.h): the gapped passes of batches of long reads - their searches do not use the wave's
  // LDS slot, which the filter cuts into one region per read of the wave (XM_BOUND_REGIONS: planLaunch); reads that do not align spend 83 % of their search nodes
  // in searches it proves null
  bool filterAllowed(bool heavy, int scale) const { return heavy && boundFilterOn && scale >= XM_HBM_ONLY_FROM; }
};

inline BatchPolicy makePolicy(const BatchFacts& f, const PassKnobs& k) {
  BatchPolicy p;
  p.k = k;
  p.gpuContexts = f.gpuContexts;
  p.seedScale = seedScaleOf(f.longestMate);
  p.gappedScale = (int)k.gappedScale;
  p.longReads = p.gappedScale > 4;
  p.arenaUnit = (size_t)k.arenaKb * 1024;
  p.lightTmpUnit = (size_t)k.lightTmpKb * 1024;
  p.regionBytes = (((size_t)k.regionKb * 1024 * (size_t)p.seedScale) & ~(size_t)15) + ((sizeof(SavedRead) + 15) & ~(size_t)15);
  p.scratchWanted = f.contextScratchBytes > 0 ? (unsigned long long)f.contextScratchBytes : (unsigned long long)k.scratchGib << 30;
  p.boundFilterOn = k.boundFilter && p.longReads;
  p.searchPoolOn = k.searchPool && p.gappedScale <= 4;
  return p;
}

// Passes, all on the GPU:
//  (1) light pass over every read at the seed scale: reads that reach the gapped extension chain stop with XM_ST_NEED_HEAVY
//      instead of serialising their wave;
//  (2) gapped pass over exactly those reads at the gapped scale, continued from the state the light pass saved (HandOver);
//  (3) reads whose scratch overflowed are rerun with 4x, 16x, ... the scratch.
// The work lists are built on the GPU by the lanes themselves (PassLists); every pass appends to the same result arenas.
struct PassState {
  bool heavy;               // the next launch runs the gapped chain (gapped pass and every rerun)
  int hoMode;               // HandOver::mode of the next launch
  int scale, overflowScale;
  bool orderedList;         // the next launch's list is the gapped pass's ordered one (expensive-looking reads first): only that list is dealt out lane-major
  int ts, to, tc;           // which of the two scale / out / confidence lists receives new entries
  int confRounds;
  long long nRegions;
  size_t regionsTotal;      // bytes at the start of the scratch that hold saved reads (0: none alive)
};
inline PassState firstPass(const BatchPolicy& pol) { return PassState{false, pol.k.handOver ? 1 : 0, pol.seedScale, pol.seedScale, false, 0, 0, 0, 0, 0, 0}; }

// Shape of one launch of xm_align_kernel.  Scratch layout while saved regions are alive: [region pool | lane arenas].
struct LaunchPlan {
  size_t arenaBytes;        // bytes of scratch a lane owns in this launch
  int lpw;                  // active lanes (reads) per wave
  long long nWaves;
  int grid, block;
  long long lanes;          // grid x waves per block x lpw
  long long nRegions;       // the pool of saved regions after this launch was planned (a light pass sizes it, the others find it)
  size_t regionsTotal;
  size_t scratchBytes;      // what the scratch must hold for this launch; 0: regions are alive, it cannot grow now and was sized by the light pass
  size_t gappedReserve;     // light pass: the part of scratchBytes behind the pool that is there for the gapped pass (and a plain rerun), not for this launch's lanes
  int pairLanes;            // log2 of the lanes that run a read together
  int boundFilter;          // the launch runs the rejection filter
  int boundFilterArg;       // the kernel's argument: bit 0 the filter, bit 1 the group sweep
  long long firstStride;    // gapped pass with an ordered list: the first read of every lane is dealt out (kernel), the counter starts behind those items
  unsigned long long firstItem;
  long long taperUnit;
  int poolBuffers;          // buffers of the search pool the launch wants, one per wave (0: no pool)
};

// Pure.  `budget`: bytes of scratch the context may hold now; `scratchHeld`: bytes it holds.  A caller whose allocation of scratchBytes fails halves the
// budget and plans again.
inline LaunchPlan planLaunch(const BatchPolicy& pol, const PassState& st, long long nTodo, long long nq, int numCUs, unsigned long long budget, size_t scratchHeld) {
  const PassKnobs& k = pol.k;
  const bool heavy = st.heavy;
  const int hoMode = st.hoMode, scale = st.scale;
  const size_t regionBytes = pol.regionBytes;
  LaunchPlan pl;
  size_t regionsTotal = st.regionsTotal;
  pl.nRegions = st.nRegions;
  pl.gappedReserve = 0;
  size_t arenaBytes = pol.arenaUnit * (size_t)scale;
  if (hoMode == 1) arenaBytes = pol.lightTmpUnit * (size_t)scale;                      // temporaries only (+ one region of the pool per lane / the read's own region)
  if (hoMode == 2) arenaBytes = regionBytes + pol.gappedTmpBytes(arenaBytes);          // a region for reads without saved state + temporaries
  // launch shape (measured on MI355X, profiles/r01/NOTES.md): 8 waves per SIMD worth of lanes in the light pass; the gapped chain
  // diverges inside each wave, so it runs 32 reads per wave on 4 waves per SIMD.
  // a pass over few reads spreads them over all the wave slots of the GPU (the time of a launch is its longest wave)
  const long long waveSlots = (long long)numCUs * 4 * (heavy ? k.fullWaves : k.lightWaves);
  int lpw = (int)(heavy ? k.fullLpw : k.lightLpw);
  if (heavy) lpw = (int)std::max(1ll, std::min((long long)lpw, (nTodo + waveSlots - 1) / waveSlots));
  long long lanes = waveSlots * lpw;
  if (hoMode == 1) lanes = std::min(lanes, (long long)(budget / (arenaBytes + regionBytes)));
  else if (regionsTotal > 0) lanes = std::min(lanes, (long long)((scratchHeld - regionsTotal) / arenaBytes));  // (sized by the light pass, before the pool was filled)
  else lanes = std::min(lanes, (long long)(budget / arenaBytes));
  if (lanes > nTodo) lanes = nTodo;
  // long reads, scratch for fewer lanes than asked for: fewer reads per wave before fewer waves than the GPU holds at a time (4 per SIMD) - a wave's
  // reads wait for each other's searches, an empty wave slot does nothing
  // (contexts that share the GPU share its wave slots)
  const long long slotsHeld = (long long)numCUs * 16 / std::max(1, pol.gpuContexts);
  if (heavy && pol.longReads && lpw > 1 && lanes / lpw < slotsHeld) lpw = (int)std::max(1ll, lanes / slotsHeld);
  long long nWaves = (lanes + lpw - 1) / lpw;
  if (nWaves < 1) nWaves = 1;
  if (hoMode != 1 && regionsTotal > 0) {  // the scratch cannot grow now: whole waves (and whole blocks of four) that fit behind the pool
    const long long cap = (long long)((scratchHeld - regionsTotal) / arenaBytes);
    if (cap < 1) throw std::runtime_error("the scratch behind the saved reads is smaller than one lane's arena (XM_SCRATCH_GIB / XM_ARENA_KB too small for this batch)");
    if (lpw > cap) lpw = (int)cap;
    long long w = cap / lpw;
    if (w >= 4) w &= ~3ll;
    if ((nWaves >= 4 ? ((nWaves + 3) & ~3ll) : nWaves) > w) nWaves = w;
  }
  const int block = nWaves < 4 ? (int)nWaves * 64 : 256;
  const int grid = (int)((nWaves * 64 + block - 1) / block);
  lanes = (long long)grid * (block / 64) * lpw;
  if (hoMode == 1) {
    // pool: one region per lane + one per read that may stop (at most 40 % of the scratch; reads beyond that are seeded again by the
    // gapped pass).  The scratch is sized here for the gapped pass as well: it must not move while saved regions are alive.
    // (a lane takes a fresh region only before it fetches another read, and only nTodo - lanes reads are fetched by lanes that already had one)
    // (+ some slack: lanes that see a few reads left all take a region, but only some of them get a read)
    long long extra = nTodo > lanes ? (long long)nTodo - lanes + std::min(lanes, 4096ll) : 0;
    // (long reads: a fifth - their seeding is 4 % of their time, and a gapped-pass lane of theirs is 6.7 MB: the scratch is worth more as lanes)
    extra = std::min(extra, (long long)(budget * (pol.longReads ? 1 : 2) / 5 / regionBytes) - lanes);
    extra = std::min(extra, ((long long)budget - lanes * (long long)(arenaBytes + regionBytes)) / (long long)regionBytes);
    if (extra < 0) extra = 0;
    pl.nRegions = lanes + extra;
    regionsTotal = (size_t)pl.nRegions * regionBytes;
    const size_t gappedArena = pol.arenaUnit * (size_t)pol.gappedScale, gappedLane = regionBytes + pol.gappedTmpBytes(gappedArena);
    long long gappedLanes = std::min((long long)nq, (long long)numCUs * 4 * k.fullWaves * k.fullLpw);
    gappedLanes = std::min(gappedLanes, std::max(1ll, ((long long)budget - (long long)regionsTotal) / (long long)gappedLane));
    pl.gappedReserve = std::max((size_t)gappedLanes * gappedLane, gappedArena);  // (a rerun after a full result arena runs plain, at least one lane of it)
    pl.scratchBytes = regionsTotal + std::max((size_t)lanes * arenaBytes, pl.gappedReserve) + 1024;
  } else if (regionsTotal > 0) {
    if (regionsTotal + (size_t)lanes * arenaBytes > scratchHeld) throw std::runtime_error("internal error: scratch layout (hand-over)");
    pl.scratchBytes = 0;
  } else {
    pl.scratchBytes = (size_t)lanes * arenaBytes;
  }
  pl.arenaBytes = arenaBytes; pl.lpw = lpw; pl.nWaves = nWaves; pl.grid = grid; pl.block = block; pl.lanes = lanes; pl.regionsTotal = regionsTotal;
  // two lanes per read (xm_extend.h, xmSetPairMode); eight in the passes that run the rejection filter (8 reads per wave at most): its recurrence
  // spreads a column's cells over them (XM_GROUP_LANES=0: two there as well)
  pl.pairLanes = (heavy && lpw <= 32 && k.pairLanes) ? 1 : 0;
  pl.boundFilter = (pol.filterAllowed(heavy, scale) && lpw <= XM_BOUND_REGIONS) ? 1 : 0;
  if (pl.boundFilter && pl.pairLanes && k.groupLanes) pl.pairLanes = 3;
  pl.boundFilterArg = pl.boundFilter ? (1 | (k.groupSweep ? 2 : 0)) : 0;
  const long long wavesLaunched = (long long)grid * (block / 64);
  pl.poolBuffers = (pol.searchPoolOn && heavy && scale == pol.gappedScale) ? (int)wavesLaunched : 0;
  pl.firstStride = (heavy && st.orderedList && k.heavyHint > 0 && scale == pol.gappedScale) ? wavesLaunched : 0;
  pl.firstItem = (unsigned long long)std::min((long long)nTodo, pl.firstStride * lpw);
  pl.taperUnit = heavy ? (long long)((double)nWaves * k.taperPct / 100.0) : 0ll;
  return pl;
}

// What follows a launch.  The kinds in the order they are looked for: a full result arena wins over everything (those reads run again with the same
// settings and room to spare); then the gapped pass; then the confidence rerun, but only when no scale rerun is pending (its reads may end up in that
// list too); then the scale rerun.
enum class PassKind { Done, OutRerun, Gapped, ConfRerun, ScaleRerun };
struct NextPass {
  PassKind kind;
  long long nTodo;
  int list;   // OutRerun / ConfRerun / ScaleRerun: the half of the double-buffered list the next launch reads (Gapped: the heavy list, with the late one appended)
  int clear;  // ... and the half it files into, whose count the caller clears (Gapped: nHeavy and nHeavyLate)
};
// `st` is the state the launch ran with; it becomes the next launch's.  The side effects (appending the late list, growing the result arenas, absorbing
// the confidence misses, clearing the counts) are the caller's, driven by the returned value.
inline NextPass nextPass(const BatchPolicy& pol, PassState& st, const PassCtl& ctl) {
  const bool consumed = st.hoMode == 2;
  st.orderedList = false;
  st.hoMode = 0;                           // (the gapped pass below switches to 2; reruns run plain)
  if (consumed) st.regionsTotal = 0;       // the saved reads have all been consumed
  const unsigned long long pendingHeavy = ctl.nHeavy + ctl.nHeavyLate, pendingScale = ctl.nScale[st.ts];
  const unsigned long long pendingConf = ctl.nConf[st.tc];  // (accumulates over the passes until the list is run)
  if (ctl.nOut[st.to] > 0) {  // result arena too small
    const NextPass np{PassKind::OutRerun, (long long)ctl.nOut[st.to], st.to, st.to ^ 1};
    st.to ^= 1;
    return np;
  }
  if (pendingHeavy > 0) {
    // the gapped pass runs at scale 4 straight away: far fewer lanes are needed than in the light pass, and most reads whose
    // gapped search outgrows the scale-1 scratch then finish here instead of costing one more (latency-bound) pass
    st.orderedList = true;  // one list: the expensive-looking reads first, the others behind them
    st.scale = pol.gappedScale;
    if (st.overflowScale < pol.gappedScale) st.overflowScale = pol.gappedScale;
    st.heavy = true;
    if (st.regionsTotal > 0) st.hoMode = 2;
    return NextPass{PassKind::Gapped, (long long)pendingHeavy, 0, 0};
  }
  if (pendingScale == 0 && pendingConf > 0) {
    // reads that met a (penalty, length) the confidence table did not hold: the host evaluates the keys they left (its libm, the oracle's)
    // and they run again, start to finish, in a pass of their own
    if (++st.confRounds > 1024) throw std::runtime_error("internal error: the confidence table does not converge");
    const NextPass np{PassKind::ConfRerun, (long long)pendingConf, st.tc, st.tc ^ 1};
    st.tc ^= 1;
    st.regionsTotal = 0;
    if (st.scale < pol.gappedScale) st.scale = pol.gappedScale;
    if (st.overflowScale < st.scale) st.overflowScale = st.scale;
    st.heavy = true;
    return np;
  }
  if (pendingScale == 0) return NextPass{PassKind::Done, 0, 0, 0};
  const NextPass np{PassKind::ScaleRerun, (long long)pendingScale, st.ts, st.ts ^ 1};
  st.ts ^= 1;
  st.regionsTotal = 0;  // (no gapped pass ran: whatever the light pass saved is not wanted any more)
  st.overflowScale *= 4;
  st.scale = st.overflowScale;
  st.heavy = true;
  if (st.scale > 4096) throw std::runtime_error("Failed to align: scratch scale limit reached (query needs more than 4096x the default scratch)");
  return np;
}

}  // namespace xm
