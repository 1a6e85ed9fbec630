// The plan and the table logic of the run-wide memory of aligned queries (xm_context_set_memo; DESIGN.md "Identical queries"), as plain C++: what a
// byte budget buys, the size of a record, when insertion stops, when the memory is emptied, and the probe / claim / dead-slot rules of the
// open-addressing table.  The kernels of xm_memo.h call the same functions on the device (they are host+device there, and plain inline functions
// everywhere else), so tests/test_memo_plan.py checks without a GPU the very code the GPU runs.  No HIP, no threads.
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

}  // namespace xm
