// Stand-alone driver of the generations of mapper_amd/csrc/xm_memo_plan.h ("the memory of a GPU") for tests/test_memo_generations.py: a memory of one or two
// generations run on the host with the very functions the kernels of xm_memo.h and the host code of xm_capi.hip call (memoLookupGenerations, memoPromotes,
// memoPromoteClaim, memoMustTurn, memoTurn, memoInsertCount, memoClaim, memoReserve), one align call at a time in the order xm_capi.hip runs it: lookup,
// promotion, (the passes,) measure, turn, insert.  Commands on stdin, answers on stdout:
//   plan <budget> <generations>                     -> slots arenaBytes capacity minBytes      (of one generation; 0 0 0: refused)
//   takes <budget> <claimed> <cursor> <n> <bytes>   -> 0 | 1                                   (memoTakesAll on memoPlan(budget))
//   new <budget> <generations> <bits>               -> ok | refused
//   empty                                           -> ok                                      (a change of parameters: every generation emptied)
//   call <k>, then k lines <hex fingerprint> <content id> <len0> <len1> <intLen> <dblLen>  (the call's representatives: different queries)
//       -> k lookup answers: "Y <offset>" (served from the young generation) | "O <offset>" (from the old one) | "-" (a miss); offsets are of the whole arena
//       -> "promote <records copied>" | "promote none"
//       -> "turn" | "stay"
//       -> one answer per miss, in order: stored <offset> | dropped | dead | skipped
//       -> "state <young> <claimed0> <cursor0> <records0> <claimed1> <cursor1> <records1> <turns> <promoted> <held> <bytes in use>"
#include "../mapper_amd/csrc/xm_memo_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace xm;

struct Item { unsigned long long fp; unsigned long long content; int len0, len1, intLen, dblLen; };

static uint8_t byteOf(unsigned long long content, int i) { return (uint8_t)((content * 0x9E3779B97F4A7C15ull + (unsigned long long)i * 0xBF58476D1CE4E5B9ull) >> 56); }
static unsigned long long casOf(unsigned long long* a, unsigned long long expected, unsigned long long desired) {
  const unsigned long long was = *a;
  if (was == expected) *a = desired;
  return was;
}
static unsigned long long addOf(unsigned long long* a, unsigned long long k) {
  const unsigned long long was = *a;
  *a += k;
  return was;
}

struct Memory {
  MemoPlan plan{0, 0, 0};
  MemoGenerations gens;
  int bits = 64;
  std::vector<unsigned long long> keys, offs, state;  // [generations * slots], [generations * slots], [generations * 4]
  std::vector<uint8_t> arena;                         // [generations * arenaBytes]
  unsigned long long mask() const { return (unsigned long long)plan.slots - 1; }
  unsigned long long* keysOf(int g) { return keys.data() + (size_t)g * (size_t)plan.slots; }
  unsigned long long* offsOf(int g) { return offs.data() + (size_t)g * (size_t)plan.slots; }
  unsigned long long* stateOf(int g) { return state.data() + (size_t)g * 4; }
  uint8_t* arenaOf(int g) { return arena.data() + (size_t)g * (size_t)plan.arenaBytes; }
  static MemoHeader headerOf(const Item& it) {
    MemoHeader h;
    memset(&h, 0, sizeof(h));
    h.mateCount = it.len1 > 0 ? 2 : 1; h.len0 = it.len0; h.len1 = it.len1; h.intLen = it.intLen; h.dblLen = it.dblLen;
    h.innerBits = it.content >> 7; h.deviationBits = it.content << 3;
    return h;
  }
  void emptyGeneration(int g) {  // Memory::clearGeneration of xm_capi.hip
    for (long long i = 0; i < plan.slots; i++) { keysOf(g)[i] = 0; offsOf(g)[i] = XM_MEMO_DEAD; }
    for (int i = 0; i < 4; i++) stateOf(g)[i] = 0;
    memoEmptyGeneration(gens, g);
  }
  void readState(int g) { gens.claimed[g] = stateOf(g)[0]; gens.cursor[g] = stateOf(g)[1]; gens.records[g] = stateOf(g)[2]; }
  // the comparison of xm_memo_lookup_kernel: header and bytes; the slices must be the ones stored for this content
  bool sameAt(long long at, const Item& it, bool* corrupt) const {
    const MemoHeader want = headerOf(it);
    MemoHeader hd;
    memcpy(&hd, arena.data() + at, sizeof(hd));
    bool same = hd.mateCount == want.mateCount && hd.len0 == want.len0 && hd.len1 == want.len1 && hd.innerBits == want.innerBits && hd.deviationBits == want.deviationBits;
    for (int i = 0; same && i < hd.len0 + hd.len1; i++) same = arena[(size_t)at + memoBytesAt(hd) + i] == byteOf(it.content, i);
    if (!same) return false;
    for (int i = 0; i < hd.intLen; i++) { int32_t v; memcpy(&v, arena.data() + at + memoIntsAt(hd) + 4 * (size_t)i, 4); if (v != (int32_t)(it.content + (unsigned)i)) *corrupt = true; }
    for (int i = 0; i < hd.dblLen; i++) { double v; memcpy(&v, arena.data() + at + memoDblsAt(hd) + 8 * (size_t)i, 8); if (v != (double)it.content + i) *corrupt = true; }
    return true;
  }
  // xm_memo_insert_kernel, one item into the young generation
  std::string insertOne(const Item& it) {
    const int g = gens.young;
    const MemoHeader hd = headerOf(it);
    const long long slot = memoClaim(keysOf(g), mask(), memoFingerprint(it.fp, bits), casOf);
    if (slot < 0) return "dropped";
    stateOf(g)[0]++;
    const unsigned long long at = memoReserve(&stateOf(g)[1], (unsigned long long)plan.arenaBytes, memoRecordBytes(hd), addOf);
    if (at == XM_MEMO_DEAD) return "dead";
    stateOf(g)[2]++;
    uint8_t* rec = arenaOf(g) + at;
    memcpy(rec, &hd, sizeof(hd));
    for (int i = 0; i < it.len0 + it.len1; i++) rec[memoBytesAt(hd) + i] = byteOf(it.content, i);
    for (int i = 0; i < it.intLen; i++) { const int32_t v = (int32_t)(it.content + (unsigned)i); memcpy(rec + memoIntsAt(hd) + 4 * (size_t)i, &v, 4); }
    for (int i = 0; i < it.dblLen; i++) { const double v = (double)it.content + i; memcpy(rec + memoDblsAt(hd) + 8 * (size_t)i, &v, 8); }
    offsOf(g)[slot] = at;
    return "stored " + std::to_string((unsigned long long)g * (unsigned long long)plan.arenaBytes + at);
  }
  // xm_memo_promote_kernel, one record of the old generation
  bool promoteOne(long long at, unsigned long long fp) {
    const int g = gens.young;
    MemoHeader hd;
    memcpy(&hd, arena.data() + at, sizeof(hd));
    const unsigned long long bytes = memoRecordBytes(hd);
    long long slot = -1;
    const unsigned long long to = memoPromoteClaim(keysOf(g), mask(), stateOf(g), (unsigned long long)plan.arenaBytes, fp, bytes, casOf, addOf, &slot);
    if (to == XM_MEMO_DEAD) return false;
    memcpy(arenaOf(g) + to, arena.data() + at, (size_t)bytes);
    offsOf(g)[slot] = to;
    return true;
  }
};

int main() {
  Memory m;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "plan") {
      long long budget; int generations;
      in >> budget >> generations;
      const MemoPlan p = memoGenerationPlan(budget, generations);
      printf("%lld %lld %lld %lld\n", p.slots, p.arenaBytes, p.capacity, memoMinBytes(generations));
    } else if (cmd == "takes") {
      long long budget; unsigned long long claimed, cursor, n, bytes;
      in >> budget >> claimed >> cursor >> n >> bytes;
      printf("%d\n", memoTakesAll(memoPlan(budget), claimed, cursor, n, bytes) ? 1 : 0);
    } else if (cmd == "new") {
      long long budget; int generations;
      in >> budget >> generations >> m.bits;
      m.plan = memoGenerationPlan(budget, generations);
      if (m.plan.slots == 0) { printf("refused\n"); continue; }
      const size_t g = (size_t)generations;
      m.keys.assign(g * (size_t)m.plan.slots, 0ull); m.offs.assign(g * (size_t)m.plan.slots, XM_MEMO_DEAD); m.state.assign(g * 4, 0ull);
      m.arena.assign(g * (size_t)m.plan.arenaBytes, 0);
      m.gens = MemoGenerations();
      m.gens.generations = generations;
      printf("ok\n");
    } else if (cmd == "empty") {
      for (int g = 0; g < m.gens.generations; g++) m.emptyGeneration(g);
      printf("ok\n");
    } else if (cmd == "call") {
      long long k;
      in >> k;
      std::vector<Item> items((size_t)k);
      for (Item& it : items) {
        std::getline(std::cin, line);
        std::istringstream li(line);
        std::string hex;
        li >> hex >> it.content >> it.len0 >> it.len1 >> it.intLen >> it.dblLen;
        it.fp = strtoull(hex.c_str(), nullptr, 16);
      }
      // memoLookup of xm_capi.hip: every representative through the generations, the old-only hits counted with their bytes
      std::vector<long long> hit((size_t)k, -1);
      std::vector<unsigned long long> fp((size_t)k, 0);
      unsigned long long oldHits = 0, oldHitBytes = 0;
      bool corrupt = false;
      for (size_t i = 0; i < items.size(); i++) {
        fp[i] = memoFingerprint(items[i].fp, m.bits);
        int generation = m.gens.young;
        hit[i] = memoLookupGenerations(m.keys.data(), m.offs.data(), m.mask(), (unsigned long long)m.plan.arenaBytes, m.gens.generations, m.gens.young, fp[i],
                                       [&](long long at) { return m.sameAt(at, items[i], &corrupt); }, &generation);
        if (hit[i] < 0) { printf("-\n"); continue; }
        if (memoGenerationOf((unsigned long long)hit[i], (unsigned long long)m.plan.arenaBytes) != generation) corrupt = true;
        printf("%s %lld\n", generation == m.gens.young ? "Y" : "O", hit[i]);
        if (generation != m.gens.young) {
          MemoHeader hd;
          memcpy(&hd, m.arena.data() + hit[i], sizeof(hd));
          oldHits++; oldHitBytes += memoRecordBytes(hd);
        }
      }
      if (corrupt) { printf("corrupt\n"); return 3; }
      // memoPromote
      if (memoPromotes(m.plan, m.gens, oldHits, oldHitBytes)) {
        long long copied = 0;
        for (size_t i = 0; i < items.size(); i++)
          if (hit[i] >= 0 && memoGenerationOf((unsigned long long)hit[i], (unsigned long long)m.plan.arenaBytes) != m.gens.young && m.promoteOne(hit[i], fp[i])) copied++;
        m.readState(m.gens.young);
        m.gens.promoted += copied;
        printf("promote %lld\n", copied);
      } else {
        printf("promote none\n");
      }
      // memoInsert: measure, turn, insert
      std::vector<size_t> misses;
      unsigned long long n = 0, bytes = 0;
      for (size_t i = 0; i < items.size(); i++)
        if (hit[i] < 0) { misses.push_back(i); n++; bytes += memoRecordBytes(Memory::headerOf(items[i])); }
      if (!misses.empty() && memoMustTurn(m.plan, m.gens, n, bytes)) {
        m.emptyGeneration(memoTurn(m.gens));
        printf("turn\n");
      } else {
        printf("stay\n");
      }
      const long long take = misses.empty() ? 0 : memoInsertCount(m.plan, m.gens, (long long)misses.size());
      for (size_t j = 0; j < misses.size(); j++) printf("%s\n", (long long)j < take ? m.insertOne(items[misses[j]]).c_str() : "skipped");
      m.readState(m.gens.young);
      printf("state %d %llu %llu %llu %llu %llu %llu %lld %lld %llu %llu\n", m.gens.young, m.gens.claimed[0], m.gens.cursor[0], m.gens.records[0], m.gens.claimed[1], m.gens.cursor[1],
             m.gens.records[1], m.gens.turns, m.gens.promoted, memoRecordsHeld(m.gens), memoBytesInUse(m.plan, m.gens));
    } else if (!cmd.empty()) {
      printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
