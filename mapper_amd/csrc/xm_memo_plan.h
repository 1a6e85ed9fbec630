// The plan and the table logic of the run-wide memory of aligned queries (xm_context_set_memo, xm_memory_new; DESIGN.md "Identical queries"), as plain C++: what a
// byte budget buys, the size of a record, when insertion stops, when the memory is emptied, the probe / claim / dead-slot rules of the
// open-addressing table, and - at the end of the file - the generations of a shared memory: lookup order, turn, promotion.  The kernels of xm_memo.h call the same functions on the device (they are host+device there, and plain inline functions
// everywhere else), so tests/test_memo_plan.py and tests/test_memo_generations.py check without a GPU the very code the GPU runs.  No HIP, no threads.
//
// The table: keys[slots] (0 = empty) and offs[slots], slots a power of two.  A slot's key is written once, by a compare-and-swap that claims it, and
// never changes until the whole memory is emptied.  offs[slot] is the record's offset in the byte arena, or XM_MEMO_DEAD: the slot is taken and
// matches nothing (its record found no room in the arena).  A key is in the table at most once: whoever meets its own key on the way drops what it
// brought (two different queries with one fingerprint: the first stays, the second is never remembered and always aligned).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XM_MEMO_FN __host__ __device__ __forceinline__
#else
#define XM_MEMO_FN inline
#endif

namespace xm {

constexpr unsigned long long XM_MEMO_DEAD = ~0ull;          // offs[slot]: taken, never matching (also what a freshly emptied table holds)
constexpr long long XM_MEMO_SLOT_BYTES = 16;                // a key and an offset
constexpr long long XM_MEMO_MIN_BYTES = 64 << 10;           // below this budget the setter fails: 1 024 slots and 48 KiB of records
constexpr long long XM_MEMO_MAX_SLOTS = 1ll << 32;

// ---- what a byte budget buys: the table gets at most a quarter of it (the largest power of two of slots that fits a quarter), the arena the rest, rounded
// down to the records' alignment.  A 150-base read's record is ~0.4 KiB and costs two slots (32 bytes) at the half-full limit below, so the arena fills first.
struct MemoPlan {
  long long slots;       // power of two; 0: the budget is refused
  long long arenaBytes;  // multiple of 8
  long long capacity;    // entries the table takes: slots / 2
};
inline MemoPlan memoPlan(long long budgetBytes) {
  MemoPlan p{0, 0, 0};
  if (budgetBytes < XM_MEMO_MIN_BYTES) return p;
  long long slots = 64;
  while (slots * 2 * XM_MEMO_SLOT_BYTES <= budgetBytes / 4 && slots * 2 <= XM_MEMO_MAX_SLOTS) slots *= 2;
  p.slots = slots;
  p.arenaBytes = (budgetBytes - slots * XM_MEMO_SLOT_BYTES) & ~7ll;
  p.capacity = slots / 2;
  return p;
}
inline long long memoTableBytes(const MemoPlan& p) { return p.slots * XM_MEMO_SLOT_BYTES; }

// ---- a record: header, the mates' bytes, the int slice, the double slice; every part starts on a multiple of 8
struct MemoHeader {
  int32_t mateCount, len0, len1;  // (len1 = 0 for a single read)
  int32_t intLen, dblLen;         // elements of the two slices
  int32_t reserved;
  unsigned long long innerBits, deviationBits;  // bit patterns of expected_inner and deviation
};
static_assert(sizeof(MemoHeader) == 40, "MemoHeader is part of the arena's layout");
XM_MEMO_FN unsigned long long memoPad8(unsigned long long n) { return (n + 7ull) & ~7ull; }
XM_MEMO_FN unsigned long long memoBytesAt(const MemoHeader& h) { return sizeof(MemoHeader); }                              // the mates' bytes, mate 0 then mate 1
XM_MEMO_FN unsigned long long memoIntsAt(const MemoHeader& h) { return memoBytesAt(h) + memoPad8((unsigned long long)h.len0 + (unsigned long long)h.len1); }
XM_MEMO_FN unsigned long long memoDblsAt(const MemoHeader& h) { return memoIntsAt(h) + memoPad8(4ull * (unsigned long long)h.intLen); }
XM_MEMO_FN unsigned long long memoRecordBytes(const MemoHeader& h) { return memoDblsAt(h) + 8ull * (unsigned long long)h.dblLen; }

// ---- when insertion stops.  Linear probing ends at an empty slot, so at most half the slots are ever claimed: the host hands a launch no more queries than
// memoRoom().  The arena's cursor only grows; a record that does not fit leaves its slot dead and the cursor beyond the arena, so that nothing fits after it:
// full means nothing more is remembered (there is no eviction).
inline long long memoRoom(const MemoPlan& p, unsigned long long claimed) { return (long long)claimed >= p.capacity ? 0 : p.capacity - (long long)claimed; }
inline bool memoFull(const MemoPlan& p, unsigned long long claimed, unsigned long long cursor) { return memoRoom(p, claimed) == 0 || cursor >= (unsigned long long)p.arenaBytes; }
inline unsigned long long memoArenaUsed(const MemoPlan& p, unsigned long long cursor) { return cursor < (unsigned long long)p.arenaBytes ? cursor : (unsigned long long)p.arenaBytes; }

// ---- when the memory is emptied: a stored result depends on the alignment parameters, so a call whose parameters differ in any bit from the ones the
// memory was filled under empties it before it looks anything up.  (A memory nothing was put into has no parameters yet and takes the call's.)
inline bool memoMustEmpty(bool filled, const void* filledUnder, const void* now, size_t bytes) { return filled && memcmp(filledUnder, now, bytes) != 0; }

// ---- the memory's fingerprint: the collapse's 64 bits, or only the lowest `bits` of them (XM_MEMO_FINGERPRINT_BITS, a test knob: 64-bit fingerprints never
// collide in a test).  Never 0, which marks an empty slot.
XM_MEMO_FN unsigned long long memoFingerprint(unsigned long long h, int bits) {
  if (bits > 0 && bits < 64) h &= (1ull << bits) - 1ull;
  return h == 0 ? 1ull : h;
}

// ---- probe: the slot that holds key h, or -1 when the probe meets an empty slot first.  Plain loads: a lookup only runs in launches after the ones that
// wrote the keys.
XM_MEMO_FN long long memoProbe(const unsigned long long* keys, unsigned long long mask, unsigned long long h) {
  unsigned long long slot = h & mask;
  for (unsigned long long n = 0; n <= mask; n++) {  // (at most half the slots are taken: the probe ends long before)
    const unsigned long long k = keys[slot];
    if (k == h) return (long long)slot;
    if (k == 0) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}
// what a probe's slot gives: the record's offset, or -1 for a dead slot
XM_MEMO_FN long long memoSlotRecord(const unsigned long long* offs, long long slot) {
  if (slot < 0) return -1;
  const unsigned long long o = offs[slot];
  return o == XM_MEMO_DEAD ? -1 : (long long)o;
}

// ---- claim: the first empty slot of h's probe sequence becomes h's (-> the slot), unless h is met on the way (-> -1: the query is dropped).  cas(address,
// expected, desired) returns what was there: a device-scope atomicCAS in the kernel, a plain compare-and-swap in the host model.
template <class Cas>
XM_MEMO_FN long long memoClaim(unsigned long long* keys, unsigned long long mask, unsigned long long h, Cas cas) {
  unsigned long long slot = h & mask;
  for (unsigned long long n = 0; n <= mask; n++) {
    const unsigned long long was = cas(&keys[slot], 0ull, h);
    if (was == 0) return (long long)slot;
    if (was == h) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;  // (a table without an empty slot: never reached, memoRoom keeps half of them empty)
}

// ---- reserve: room for a record of `bytes` from the arena's cursor.  add(address, n) returns the value before (atomicAdd).  -> the offset, or
// XM_MEMO_DEAD when the record does not fit: the claimed slot keeps that value, which a freshly emptied table holds everywhere.
template <class Add>
XM_MEMO_FN unsigned long long memoReserve(unsigned long long* cursor, unsigned long long arenaBytes, unsigned long long bytes, Add add) {
  const unsigned long long at = add(cursor, bytes);
  return (at + bytes <= arenaBytes && at + bytes >= at) ? at : XM_MEMO_DEAD;
}

// ================================================================ the memory of a GPU (xm_memory_new): one or two generations
// A memory that several contexts share, and that keeps remembering however long the run is, is one or two tables as above - GENERATIONS - in one
// allocation each of keys, offsets, records and state words: generation g has keys[g * slots ..), offs[g * slots ..), the arena's bytes
// [g * arenaBytes ..) and state[g * 4 ..), so a record's offset in the whole arena (what hit[q] holds) says which generation it is in.  One generation
// is the YOUNG one: inserts go there.  The other, if there is one, is the OLD one: it is only read.  A TURN drops the old generation, makes the
// young one the old one, and the dropped one, emptied, the young one.  With one generation nothing ever turns: full means nothing more is remembered.
constexpr int XM_MEMO_MAX_GENERATIONS = 2;

// ---- the plan: every generation is memoPlan(budget / generations); slots == 0: refused (generations other than 1 or 2, or less than generations * XM_MEMO_MIN_BYTES)
inline long long memoMinBytes(int generations) { return (long long)generations * XM_MEMO_MIN_BYTES; }
inline MemoPlan memoGenerationPlan(long long budgetBytes, int generations) {
  if (generations < 1 || generations > XM_MEMO_MAX_GENERATIONS || budgetBytes < 0) return MemoPlan{0, 0, 0};
  return memoPlan(budgetBytes / generations);
}

// ---- what the host knows of the generations: its copy of each one's state words after the last launch that changed them, which one is young, the counts
struct MemoGenerations {
  int generations = 1;
  int young = 0;
  unsigned long long claimed[XM_MEMO_MAX_GENERATIONS] = {0, 0}, cursor[XM_MEMO_MAX_GENERATIONS] = {0, 0}, records[XM_MEMO_MAX_GENERATIONS] = {0, 0};
  long long turns = 0, promoted = 0;
};
XM_MEMO_FN int memoOldOf(int generations, int young) { return generations > 1 ? 1 - young : -1; }  // (-1: there is none)
XM_MEMO_FN int memoGenerationOf(unsigned long long at, unsigned long long arenaBytes) { return (int)(at / arenaBytes); }  // of a record's offset in the whole arena
inline unsigned long long memoRecordsHeld(const MemoGenerations& g) { return g.records[0] + (g.generations > 1 ? g.records[1] : 0ull); }
inline unsigned long long memoBytesInUse(const MemoPlan& p, const MemoGenerations& g) {
  unsigned long long b = 0;
  for (int k = 0; k < g.generations; k++) b += (unsigned long long)memoTableBytes(p) + memoArenaUsed(p, g.cursor[k]);
  return b;
}
inline void memoEmptyGeneration(MemoGenerations& g, int k) { g.claimed[k] = g.cursor[k] = g.records[k] = 0; }

// ---- lookup order: the young generation first, then the old one.  same(at) says whether the record at offset `at` of the whole arena is this query,
// byte for byte.  A key match whose record is another query (two queries, one fingerprint) does not end the lookup: the other generation is still
// probed.  A query held in both generations is served from the young one.  -> the record's offset in the whole arena (*generation: where), or -1
template <class Same>
XM_MEMO_FN long long memoLookupGenerations(const unsigned long long* keys, const unsigned long long* offs, unsigned long long mask, unsigned long long arenaBytes, int generations, int young,
                                           unsigned long long h, Same same, int* generation) {
  for (int k = 0; k < generations && k < XM_MEMO_MAX_GENERATIONS; k++) {
    const int g = k == 0 ? young : 1 - young;
    const unsigned long long* gk = keys + (unsigned long long)g * (mask + 1);
    const unsigned long long* go = offs + (unsigned long long)g * (mask + 1);
    const long long rec = memoSlotRecord(go, memoProbe(gk, mask, h));
    if (rec < 0) continue;
    const long long at = (long long)((unsigned long long)g * arenaBytes) + rec;
    if (same(at)) { *generation = g; return at; }
  }
  return -1;
}

// ---- insert.  Before the insert of a call the exact number n of representatives it aligned and the exact sum B of their memoRecordBytes are known
// (xm_memo_measure_kernel).  The young generation takes all of them, or - with two generations and a young one that holds something - the generations
// turn first and the insert goes to the fresh young one.  A batch larger than a whole generation is inserted as far as room goes (memoRoom, memoFull,
// memoReserve: which of its queries fit is then not determined).
inline bool memoTakesAll(const MemoPlan& p, unsigned long long claimed, unsigned long long cursor, unsigned long long n, unsigned long long bytes) {
  return claimed + n <= (unsigned long long)p.capacity && cursor + bytes <= (unsigned long long)p.arenaBytes && cursor + bytes >= cursor;
}
inline bool memoMustTurn(const MemoPlan& p, const MemoGenerations& g, unsigned long long n, unsigned long long bytes) {
  return g.generations > 1 && g.claimed[g.young] > 0 && !memoTakesAll(p, g.claimed[g.young], g.cursor[g.young], n, bytes);
}
// the turn, on the host's copy: -> the generation the caller has to empty in HBM (it is the young one now)
inline int memoTurn(MemoGenerations& g) {
  g.young = 1 - g.young;
  memoEmptyGeneration(g, g.young);
  g.turns++;
  return g.young;
}
// how many of a call's k aligned representatives the insert launch is given (the first ones of its list)
inline long long memoInsertCount(const MemoPlan& p, const MemoGenerations& g, long long k) {
  if (memoFull(p, g.claimed[g.young], g.cursor[g.young])) return 0;
  const long long room = memoRoom(p, g.claimed[g.young]);
  return k < room ? k : room;
}

// ---- promotion (second chance).  The lookup counts the hits it found in the old generation only, and the exact bytes of their records.  If the young
// generation takes all of them, xm_memo_promote_kernel copies those records into it (claim the key, reserve room, copy the record verbatim; a promotion
// that meets its own key in the young table is dropped); otherwise none is promoted in this call.  Promotion never turns the generations.
inline bool memoPromotes(const MemoPlan& p, const MemoGenerations& g, unsigned long long oldHits, unsigned long long oldHitBytes) {
  return g.generations > 1 && oldHits > 0 && memoTakesAll(p, g.claimed[g.young], g.cursor[g.young], oldHits, oldHitBytes);
}
// one record's promotion: -> its offset in the young generation's arena, or XM_MEMO_DEAD (dropped).  *slot: the claimed slot of the young table; the
// caller copies memoRecordBytes from the old record and then sets offs[*slot].
template <class Cas, class Add>
XM_MEMO_FN unsigned long long memoPromoteClaim(unsigned long long* youngKeys, unsigned long long mask, unsigned long long* youngState, unsigned long long arenaBytes, unsigned long long h,
                                               unsigned long long bytes, Cas cas, Add add, long long* slot) {
  *slot = memoClaim(youngKeys, mask, h, cas);
  if (*slot < 0) return XM_MEMO_DEAD;
  add(&youngState[0], 1ull);
  const unsigned long long at = memoReserve(&youngState[1], arenaBytes, bytes, add);
  if (at != XM_MEMO_DEAD) add(&youngState[2], 1ull);
  return at;
}

}  // namespace xm
