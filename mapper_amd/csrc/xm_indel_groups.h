// The pile-up's insertion / deletion events grouped on the device as the batches come in (included once, by xm_capi_pileup.h): a table per
// pile-up in HBM that outlives the calls, and the kernels over the plain rules of xm_indel_groups_rules.h.  The table: open addressing over the fingerprints
// (keys[cap], cap a power of two, at most half full), per slot a word that names its group (words[cap]), an array of group records and an arena of the
// groups' letters.  The kernels work over items - the events of a call, or the groups of another pile-up.  One call folds n items in separate launches on one
// stream; no launch reads with plain loads what another workgroup of the same launch stored (the XCDs' L2s are not coherent within a launch): inside a launch
// only device-scope atomics are shared.
//   claim    a lane per item: CAS on keys[] with linear probing past other fingerprints, and an atomic min of the item's index on the slot's word, which names
//            the call's representative where the slot has no group yet - once per distinct fingerprint of the wavefront, not per lane
//   mark     every item reads its slot's word: it is the representative or it is not; the representatives' letters are measured (8-byte steps in the arena)
//   scan     exclusive sums over the representatives and over their letters: the scan of xm_pileup_text.h, run twice
//   place    a representative writes its group's record, copies its letters into the arena and leaves the group's index in the slot's word
//   add      every item compares its key with its slot's group, letters included: equal - its weight is added, one atomic add per distinct slot of the
//            wavefront; different - a true fingerprint collision: the item is left over and counted
//   left     only when something was left over: two more scans, and the left-over items written as events with their text, packed, for the host
// Nothing the size of the table is cleared per call (xm_indel_groups_rules.h: the words), and the table, the records and the arena grow before the launches,
// never inside one: the host knows the items of the call and keeps the number of groups.  The fingerprint decides how much is left to the host, never the
// output.  At the end a lane per group judges it (xm_mutations_rules.h) and the kept ones are packed for the host.
#pragma once
#include "xm_indel_groups_rules.h"
#include "xm_mutations_rules.h"
#include "xm_pileup_text.h"
#include <hip/hip_runtime.h>

namespace {

// ctl[0] items left over by the add; ctl[1] groups made by the call; ctl[2] arena bytes they took; ctl[3] representatives that found no place (must stay 0)
constexpr int XM_IGROUPS_CTL_WORDS = 4;

// The items of a fold.  Events (groups null): event i is events[8 i ..], its letters text[off[i] .. off[i + 1]).  Groups (events null): groups[i] with arena.
struct IGroupsItems {
  const long long* events; const int64_t* off; const char* text;
  const xm::IndelGroup* groups; const char* arena;
  long long n;
};
struct IGroupsTable {
  unsigned long long* keys; unsigned long long* words; unsigned long long mask;
  xm::IndelGroup* groups; char* arena;
};

// item i (i < v.n); false: it is not grouped (an event near a query end)
__device__ __forceinline__ bool igroupsItemAt(const IGroupsItems& v, long long i, xm::IndelItem& it) {
  if (v.events) {
    const long long* ev = v.events + i * xm::XM_IGROUPS_EVENT_WORDS;
    const long long lo = v.off[i], hi = v.off[i + 1];
    it = xm::indelItemOfEvent(ev, v.text + lo, hi > lo ? hi - lo : 0);
    return xm::indelGrouped(ev[5]);
  }
  it = xm::indelItemOfGroup(v.groups[i], v.arena);
  return true;
}

__global__ void __launch_bounds__(256) xm_igroups_claim_kernel(IGroupsItems v, int bits, IGroupsTable table, long long* slotOf) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long h = 0;
  if (i < v.n) {  // (lanes behind the last item stay for the ballots and claim nothing)
    xm::IndelItem it;
    if (igroupsItemAt(v, i, it)) h = xm::indelFingerprint(it, bits);  // (never 0)
  }
  // One claim per distinct fingerprint of the wavefront: the lowest live lane - the lowest item of its fingerprint here, since items ascend with the lanes -
  // probes, claims and asks to be the representative, and the lanes with the same fingerprint take its slot.  Deep coverage sends many events of a wavefront
  // to one slot.
  long long slot = -1;
  unsigned long long live = __ballot(h != 0);
  while (live) {
    const int leader = __ffsll((long long)live) - 1;
    const unsigned long long mine = __shfl(h, leader, 64);
    unsigned long long at = 0;
    if (lane == leader) {
      at = xm::indelFirstSlot(mine, table.mask);
      while (true) {  // (at most half the slots are taken: the probe ends)
        const unsigned long long was = atomicCAS(&table.keys[at], 0ull, mine);
        if (was == 0 || was == mine) break;
        at = (at + 1) & table.mask;
      }
      atomicMin(&table.words[at], xm::XM_IGROUPS_REP | (unsigned long long)i);  // (a group's index is lower and stays)
    }
    at = __shfl(at, leader, 64);
    if (h == mine) slot = (long long)at;
    live &= ~__ballot(h == mine);
  }
  if (i < v.n) slotOf[i] = slot;
}

__global__ void __launch_bounds__(256) xm_igroups_mark_kernel(IGroupsItems v, IGroupsTable table, const long long* slotOf, long long* isRep, long long* repBytes) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.n) return;
  const long long slot = slotOf[i];
  bool rep = false;
  long long bytes = 0;
  if (slot >= 0) {
    rep = table.words[slot] == (xm::XM_IGROUPS_REP | (unsigned long long)i);  // (stored by the claim launch)
    if (rep) {
      xm::IndelItem it;
      (void)igroupsItemAt(v, i, it);
      bytes = xm::indelArenaBytes(it.numLetters);
    }
  }
  isRep[i] = rep ? 1 : 0;
  repBytes[i] = bytes;
}

// groupsBase, arenaBase: the groups and the arena bytes in front of this call's; no record is written at or behind groupCap, no byte at or behind arenaCap
__global__ void __launch_bounds__(256) xm_igroups_place_kernel(IGroupsItems v, IGroupsTable table, const long long* slotOf, const long long* isRep, const int64_t* repOff, const int64_t* bytesOff,
                                                               long long groupsBase, long long arenaBase, long long groupCap, long long arenaCap, unsigned long long* ctl) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { ctl[1] = (unsigned long long)repOff[v.n]; ctl[2] = (unsigned long long)bytesOff[v.n]; }
  if (i >= v.n || !isRep[i]) return;
  xm::IndelItem it;
  (void)igroupsItemAt(v, i, it);
  const long long g = groupsBase + repOff[i], at = arenaBase + bytesOff[i], bytes = xm::indelArenaBytes(it.numLetters);
  if (g < groupsBase || g >= groupCap || at < arenaBase || at + bytes > arenaCap) { atomicAdd(&ctl[3], 1ull); return; }
  xm::IndelGroup rec;
  rec.contig = it.contig; rec.kind = it.kind; rec.pos1 = it.pos1; rec.length = it.length; rec.numLetters = it.numLetters; rec.lettersAt = at; rec.support = 0;
  table.groups[g] = rec;
  xm::indelLettersCopy(table.arena + at, it.letters, it.numLetters);
  for (long long k = it.numLetters; k < bytes; k++) table.arena[at + k] = 0;
  table.words[slotOf[i]] = (unsigned long long)g;  // (this lane alone writes the word in this launch; the add launch reads it)
}

__global__ void __launch_bounds__(256) xm_igroups_add_kernel(IGroupsItems v, IGroupsTable table, const long long* slotOf, long long groupCount, long long* leftFlag, long long* leftLen,
                                                             unsigned long long* ctl) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  bool counted = false, left = false;
  long long slot = -1;
  unsigned long long g = 0, weight = 0;
  if (i < v.n) {
    slot = slotOf[i];
    long long letters = 0;
    if (slot >= 0) {
      xm::IndelItem it;
      (void)igroupsItemAt(v, i, it);
      g = table.words[slot];  // (stored by the place launch, or by an earlier call)
      counted = g < (unsigned long long)groupCount && xm::indelSameKey(table.groups[g], table.arena, it);
      left = !counted;  // a fingerprint collision: the host groups this one
      weight = it.weight;
      letters = it.numLetters;
    }
    leftFlag[i] = left ? 1 : 0;
    leftLen[i] = left ? letters : 0;
  }
  // one add per distinct slot of the wavefront: the lanes of the lowest live lane's slot are summed and added by that lane, until no lane is live
  unsigned long long live = __ballot(counted);
  while (live) {
    const int leader = __ffsll((long long)live) - 1;
    const long long s = __shfl(slot, leader, 64);
    const unsigned long long same = __ballot(counted && slot == s);
    unsigned long long sum = counted && slot == s ? weight : 0ull;
    if (__popcll(same) > 1)
      for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == leader) atomicAdd(&table.groups[g].support, sum);
    live &= ~same;
  }
  const unsigned long long lefts = __ballot(left);
  if (lane == 0 && lefts) atomicAdd(&ctl[0], (unsigned long long)__popcll(lefts));
}

// the left-over items as events with their text, packed in item order: event lOff[i], its letters at ltOff[i]
__global__ void __launch_bounds__(256) xm_igroups_left_kernel(IGroupsItems v, const long long* leftFlag, const int64_t* lOff, const int64_t* ltOff, long long* leftEvents, long long leftCap,
                                                              int64_t* leftTextOff, char* leftText, long long textCap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && lOff[v.n] >= 0 && lOff[v.n] <= leftCap) leftTextOff[lOff[v.n]] = ltOff[v.n];
  if (i >= v.n || !leftFlag[i]) return;
  const long long at = lOff[i], t = ltOff[i];
  xm::IndelItem it;
  (void)igroupsItemAt(v, i, it);
  if (at < 0 || at >= leftCap || t < 0 || t + it.numLetters > textCap) return;
  long long* ev = leftEvents + at * xm::XM_IGROUPS_EVENT_WORDS;
  if (v.events) {
    const long long* from = v.events + i * xm::XM_IGROUPS_EVENT_WORDS;
    for (int k = 0; k < xm::XM_IGROUPS_EVENT_WORDS; k++) ev[k] = from[k];
  } else {
    xm::indelEventOfItem(it, ev);
  }
  leftTextOff[at] = t;
  xm::indelLettersCopy(leftText + t, it.letters, it.numLetters);
}

// A larger table takes the occupied slots of the old one.  The fingerprints are distinct: a lane claims a slot that no other lane of the launch looks for, and
// there is nothing to compare.
__global__ void __launch_bounds__(256) xm_igroups_regrow_kernel(const unsigned long long* oldKeys, const unsigned long long* oldWords, unsigned long long oldCap, IGroupsTable table) {
  const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= oldCap) return;
  const unsigned long long key = oldKeys[s];
  if (key == 0) return;
  unsigned long long at = xm::indelFirstSlot(key, table.mask);
  while (atomicCAS(&table.keys[at], 0ull, key) != 0) at = (at + 1) & table.mask;
  table.words[at] = oldWords[s];
}

// ---------------------------------------------------------------- the end: judge, compact, gather
// a group as the host gets it: xm_indel_call's layout (include/xmapper_hip.h)
struct IGroupsCall {
  int32_t contig, kind;
  int64_t pos1, length, keep;
  unsigned long long supportUnits, totalUnits;
  int64_t lettersAt, numLetters;
};
static_assert(sizeof(IGroupsCall) == 64, "xm_indel_call is 64 bytes");

// A lane per group.  middle null: no counts (total 0, every group kept whole).  judged 0: every group comes down, keep = length, total as judged.
__global__ void __launch_bounds__(256) xm_igroups_judge_kernel(const xm::IndelGroup* groups, long long n, const unsigned long long* middle, const int64_t* contigStart, const int32_t* contigLen,
                                                               int numContigs, xm::MutationFilter filter, int judged, long long* keep, unsigned long long* total, long long* flag, long long* letters) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const xm::IndelGroup c = groups[g];
  unsigned long long t = 0;
  long long k = 0;
  if (middle && c.contig >= 0 && c.contig < numContigs && contigLen[c.contig] >= 1)
    k = xm::mutationsJudgeIndel(middle + contigStart[c.contig], contigLen[c.contig], c.pos1, c.kind, c.length, c.support, filter, &t);
  if (!judged) k = c.length;
  const bool down = !judged || k > 0;
  keep[g] = k; total[g] = t;
  flag[g] = down ? 1 : 0;
  letters[g] = down ? c.numLetters : 0;
}

__global__ void __launch_bounds__(256) xm_igroups_gather_kernel(const xm::IndelGroup* groups, const char* arena, long long n, const long long* keep, const unsigned long long* total,
                                                                const long long* flag, const int64_t* off, const int64_t* textOff, IGroupsCall* out, long long outCap, char* text, long long textCap) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n || !flag[g]) return;
  const xm::IndelGroup c = groups[g];
  const long long at = off[g], t = textOff[g];
  if (at < 0 || at >= outCap || t < 0 || t + c.numLetters > textCap) return;
  IGroupsCall r;
  r.contig = c.contig; r.kind = c.kind; r.pos1 = c.pos1; r.length = c.length; r.keep = keep[g]; r.supportUnits = c.support; r.totalUnits = total[g]; r.lettersAt = t; r.numLetters = c.numLetters;
  out[at] = r;
  xm::indelLettersCopy(text + t, arena + c.lettersAt, c.numLetters);
}

// ---------------------------------------------------------------- the host's side
// A buffer grows and keeps its first `keep` entries: the copy is enqueued on s in front of the call's launches, and the old buffer goes to `old`, which the
// fold frees behind its own wait - growth adds no wait to a call.
template <class T>
bool igroupsGrowKeep(DevBuf<T>& b, DevBuf<T>& old, size_t keep, size_t want, hipStream_t s) {
  if (want <= b.n && b.p) return false;
  DevBuf<T> bigger;
  bigger.ensure(std::max(want, b.p ? 2 * b.n : (size_t)0));
  if (keep && b.p) HIP_CHECK(hipMemcpyAsync(bigger.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
  const bool grew = b.p != nullptr;
  old = std::move(b);
  b = std::move(bigger);
  return grew;
}

// what the host holds of the left-overs: events (8 words each) in the order they were appended, and with them their text
struct IGroupsLeft {
  std::vector<long long>* events;
  std::vector<int64_t>* textOff;
  std::vector<char>* text;
};

struct IGroupsStage {
  // the table
  DevBuf<unsigned long long> dKeys, dWords, dCtl, oldKeys, oldWords;
  DevBuf<xm::IndelGroup> dGroups, oldGroups;
  DevBuf<char> dArena, oldArena;
  unsigned long long cap = 0, leastCap = 1ull << 12;
  long long groups = 0, arenaUsed = 0;
  int bits = 64;
  long long tableGrows = 0, recordGrows = 0, arenaGrows = 0;  // (beyond the first allocation)
  long long bytesDown = 0;                                    // what the folds copied to the host
  // a call's arrays
  DevBuf<long long> dSlot, dFlag, dLen, dFlag2, dLen2, dBlocks, dLeftEvents, dKeep;
  DevBuf<unsigned long long> dTotal;
  DevBuf<int64_t> dOffA, dOffB, dLeftTextOff;
  DevBuf<char> dLeftText;
  DevBuf<IGroupsCall> dCalls;

  IGroupsTable view() { return IGroupsTable{dKeys.p, dWords.p, cap - 1, dGroups.p, dArena.p}; }

  // Room for n more items with textBytes of letters, before anything of the call is launched: capacity >= 2 (groups + n), records >= groups + n, arena >=
  // used + the call's letters in 8-byte steps.
  void reserve(long long n, long long textBytes, hipStream_t s) {
    dCtl.ensure(XM_IGROUPS_CTL_WORDS);
    const unsigned long long want = xm::indelCapacityFor((unsigned long long)groups, (unsigned long long)n, cap ? cap : leastCap);
    if (want != cap) {
      DevBuf<unsigned long long> keys, words;
      keys.ensure((size_t)want); words.ensure((size_t)want);
      HIP_CHECK(hipMemsetAsync(keys.p, 0, sizeof(unsigned long long) * (size_t)want, s));
      HIP_CHECK(hipMemsetAsync(words.p, 0xFF, sizeof(unsigned long long) * (size_t)want, s));  // (XM_IGROUPS_NONE)
      if (cap && groups) {
        const IGroupsTable bigger{keys.p, words.p, want - 1, dGroups.p, dArena.p};
        hipLaunchKernelGGL(xm_igroups_regrow_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)dKeys.p, (const unsigned long long*)dWords.p, cap, bigger);
        HIP_CHECK(hipGetLastError());
      }
      if (cap) tableGrows++;
      oldKeys = std::move(dKeys); oldWords = std::move(dWords);  // (freed by the fold, behind the kernel that reads them)
      dKeys = std::move(keys); dWords = std::move(words);
      cap = want;
    }
    if (igroupsGrowKeep(dGroups, oldGroups, (size_t)groups, (size_t)(groups + n), s)) recordGrows++;
    const long long letters = std::min<long long>(textBytes + 7 * n, 8 * textBytes);  // (every representative's letters start on an 8-byte boundary)
    if (igroupsGrowKeep(dArena, oldArena, (size_t)arenaUsed, (size_t)(arenaUsed + letters + 8), s)) arenaGrows++;
  }
  // what growth replaced, once nothing enqueued reads it any more
  void retire() {
    oldKeys = DevBuf<unsigned long long>(); oldWords = DevBuf<unsigned long long>();
    oldGroups = DevBuf<xm::IndelGroup>(); oldArena = DevBuf<char>();
  }

  // The fold of v.n > 0 items (reserve() has run for them) on stream s: one wait for the call's small record and, only when items were left over, a second
  // one for them; they are appended to `left` in the order of pileupAppendCall.  -> the items left over.
  long long fold(const IGroupsItems& v, hipStream_t s, const IGroupsLeft& left) {
    const long long n = v.n;
    const unsigned grid = (unsigned)((n + 255) / 256);
    dSlot.ensure((size_t)n); dFlag.ensure((size_t)n); dLen.ensure((size_t)n); dFlag2.ensure((size_t)n); dLen2.ensure((size_t)n); dBlocks.ensure(xmScanSums(n, 1));
    dOffA.ensure((size_t)n + 1); dOffB.ensure((size_t)n + 1);
    const IGroupsTable t = view();
    HIP_CHECK(hipMemsetAsync(dCtl.p, 0, sizeof(unsigned long long) * XM_IGROUPS_CTL_WORDS, s));
    hipLaunchKernelGGL(xm_igroups_claim_kernel, dim3(grid), dim3(256), 0, s, v, bits, t, dSlot.p);
    hipLaunchKernelGGL(xm_igroups_mark_kernel, dim3(grid), dim3(256), 0, s, v, t, (const long long*)dSlot.p, dFlag.p, dLen.p);
    HIP_CHECK(hipGetLastError());
    xmScan(XmOffsets<long long, 1>{n, {dFlag.p}, {dOffA.p}}, n, dBlocks, s);
    xmScan(XmOffsets<long long, 1>{n, {dLen.p}, {dOffB.p}}, n, dBlocks, s);
    hipLaunchKernelGGL(xm_igroups_place_kernel, dim3(grid), dim3(256), 0, s, v, t, (const long long*)dSlot.p, (const long long*)dFlag.p, (const int64_t*)dOffA.p, (const int64_t*)dOffB.p, groups,
                       arenaUsed, (long long)dGroups.n, (long long)dArena.n, dCtl.p);
    hipLaunchKernelGGL(xm_igroups_add_kernel, dim3(grid), dim3(256), 0, s, v, t, (const long long*)dSlot.p, (long long)std::min<size_t>(dGroups.n, (size_t)(groups + n)), dFlag2.p, dLen2.p, dCtl.p);
    HIP_CHECK(hipGetLastError());
    unsigned long long ctl[XM_IGROUPS_CTL_WORDS] = {0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(ctl, dCtl.p, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    retire();
    bytesDown += (long long)sizeof(ctl);
    if (ctl[3] != 0) throw std::runtime_error("internal error: " + std::to_string(ctl[3]) + " groups found no place in the table's records");
    if (ctl[1] > (unsigned long long)n || ctl[0] > (unsigned long long)n) throw std::runtime_error("internal error: more groups than items");
    groups += (long long)ctl[1];
    arenaUsed += (long long)ctl[2];
    const long long nLeft = (long long)ctl[0];
    if (nLeft == 0) return 0;
    // left-overs: true fingerprint collisions (with whole fingerprints none in any run that has been seen)
    xmScan(XmOffsets<long long, 1>{n, {dFlag2.p}, {dOffA.p}}, n, dBlocks, s);
    xmScan(XmOffsets<long long, 1>{n, {dLen2.p}, {dOffB.p}}, n, dBlocks, s);
    long long textBytes = 0;
    HIP_CHECK(hipMemcpyAsync(&textBytes, dOffB.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    dLeftEvents.ensure((size_t)nLeft * 8); dLeftTextOff.ensure((size_t)nLeft + 1); dLeftText.ensure((size_t)textBytes);
    hipLaunchKernelGGL(xm_igroups_left_kernel, dim3(grid), dim3(256), 0, s, v, (const long long*)dFlag2.p, (const int64_t*)dOffA.p, (const int64_t*)dOffB.p, dLeftEvents.p, nLeft, dLeftTextOff.p,
                       dLeftText.p, textBytes);
    HIP_CHECK(hipGetLastError());
    std::vector<long long> got((size_t)nLeft * 8);
    std::vector<int64_t> off((size_t)nLeft + 1);
    std::vector<char> text((size_t)textBytes);
    HIP_CHECK(hipMemcpyAsync(got.data(), dLeftEvents.p, sizeof(long long) * got.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(off.data(), dLeftTextOff.p, sizeof(int64_t) * off.size(), hipMemcpyDeviceToHost, s));
    if (textBytes) HIP_CHECK(hipMemcpyAsync(text.data(), dLeftText.p, (size_t)textBytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    bytesDown += (long long)(sizeof(long long) * got.size() + sizeof(int64_t) * (off.size() + 1) + (size_t)textBytes);
    if (off[(size_t)nLeft] != textBytes) throw std::runtime_error("internal error: the left-over text was measured twice with different results");
    xm::pileupAppendCall(got.data(), (size_t)nLeft, off.data(), text.data(), *left.events, left.textOff, left.text);
    return nLeft;
  }

  // the table holds nothing again (its buffers stay: the next reserve() clears the slots)
  void clear(hipStream_t s) {
    if (cap) {
      HIP_CHECK(hipMemsetAsync(dKeys.p, 0, sizeof(unsigned long long) * (size_t)cap, s));
      HIP_CHECK(hipMemsetAsync(dWords.p, 0xFF, sizeof(unsigned long long) * (size_t)cap, s));
    }
    groups = 0; arenaUsed = 0;
  }
};

}  // namespace
