// The grouping of the pile-up's insertion / deletion events, once, as plain C++: which events are grouped, the key of a group, its fingerprint
// and when two keys are equal.  pileup.MatchDatabase._indels() is the definition: an event near a query end (bit 2 of its flags word) is skipped; an insertion
// is (contig, pos1 = startB, 1, length, its kept letters), a deletion (contig, pos1 = startB + 1, 2, length) - its reference allele follows from the position
// and is the host's business - and the support of a group is the sum of its events' weights.  The kernels of xm_indel_groups.h call these functions on the
// device (they are host+device there, and plain inline functions everywhere else); tests/indel_groups_rules_main.cpp calls them on the host, so
// tests/test_indel_groups_rules.py checks without a GPU the very code the GPU runs.  No HIP, no threads, no allocation, no library call.
//
// The fingerprint decides how much is left to the host, never the output: an item is only ever added to a group whose stored key equals its own, letters
// included, byte for byte.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XM_IGROUPS_FN __host__ __device__ inline
#else
#define XM_IGROUPS_FN inline
#endif

namespace xm {

constexpr int XM_IGROUPS_EVENT_WORDS = 8;     // an event of the pile-up (include/xmapper_hip.h): contig, startB, type, length, query, flags, startA, weight
constexpr long long XM_IGROUPS_NEAR_END = 4;  // bit 2 of the flags word: the event lies near a query end

// What is folded into a table: the key (contig, pos1, kind, length, letters[0 .. numLetters)) and a weight.  The events of a call are one producer of items,
// the groups of another pile-up the other.
struct IndelItem {
  int32_t contig, kind;
  int64_t pos1, length, numLetters;
  const char* letters;
  unsigned long long weight;
};

// A group as the table holds it: the key, where its letters lie in the arena, and the summed weights.
struct IndelGroup {
  int32_t contig, kind;
  int64_t pos1, length, numLetters, lettersAt;
  unsigned long long support;
};

// whether an event with this flags word is grouped at all
XM_IGROUPS_FN bool indelGrouped(long long flags) { return (flags & XM_IGROUPS_NEAR_END) == 0; }

// the item of an event (eight words) whose kept letters are letters[0 .. numLetters) (none for a deletion)
XM_IGROUPS_FN IndelItem indelItemOfEvent(const long long* ev, const char* letters, long long numLetters) {
  IndelItem it;
  it.contig = (int32_t)ev[0];
  it.kind = (int32_t)ev[2];
  it.pos1 = ev[2] == 1 ? ev[1] : ev[1] + 1;
  it.length = ev[3];
  it.numLetters = ev[2] == 1 ? numLetters : 0;
  it.letters = letters;
  it.weight = (unsigned long long)ev[7];
  return it;
}
XM_IGROUPS_FN IndelItem indelItemOfGroup(const IndelGroup& g, const char* arena) {
  IndelItem it;
  it.contig = g.contig; it.kind = g.kind; it.pos1 = g.pos1; it.length = g.length; it.numLetters = g.numLetters;
  it.letters = arena + g.lettersAt;
  it.weight = g.support;
  return it;
}
// The event that stands for an item on the host (a left-over of a fold): grouped again by _indels() it gives the item's key and weight.  Query -1, startA 0.
XM_IGROUPS_FN void indelEventOfItem(const IndelItem& it, long long* ev) {
  ev[0] = it.contig; ev[1] = it.kind == 1 ? it.pos1 : it.pos1 - 1; ev[2] = it.kind; ev[3] = it.length;
  ev[4] = -1; ev[5] = 0; ev[6] = 0; ev[7] = (long long)it.weight;
}

XM_IGROUPS_FN unsigned long long indelMix(unsigned long long z) {  // SplitMix64's finaliser
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 64 bits over the key; only the low `bits` of them when bits < 64 (a test knob: few bits make collisions); never 0, which marks an empty slot.  The letters
// go in eight at a time, the first in the lowest byte, whatever their alignment.
XM_IGROUPS_FN unsigned long long indelFingerprint(const IndelItem& it, int bits) {
  unsigned long long h = indelMix((unsigned long long)(uint32_t)it.contig + 0x9E3779B97F4A7C15ull);
  h = indelMix(h ^ indelMix((unsigned long long)it.pos1 + 0xD1B54A32D192ED03ull));
  h = indelMix(h ^ indelMix(((unsigned long long)(uint32_t)it.kind << 56) ^ (unsigned long long)it.length));
  h = indelMix(h ^ (unsigned long long)it.numLetters);
  for (long long at = 0; at < it.numLetters; at += 8) {
    unsigned long long w = 0;
    for (int k = 0; k < 8; k++)
      if (at + k < it.numLetters) w |= (unsigned long long)(uint8_t)it.letters[at + k] << (8 * k);
    h = indelMix(h ^ indelMix(w + 0xD1B54A32D192ED03ull * (unsigned long long)(at / 8 + 1)));
  }
  if (bits >= 0 && bits < 64) h &= (1ull << bits) - 1;
  return h == 0 ? 1 : h;
}

// The widest piece (8, 4 or 1 bytes) that both addresses allow.
XM_IGROUPS_FN int indelPiece(const char* a, const char* b) {
  const uintptr_t both = (uintptr_t)a | (uintptr_t)b;
  return (both & 7) == 0 ? 8 : (both & 3) == 0 ? 4 : 1;
}

// a[0 .. n) == b[0 .. n), in the widest pieces the alignment of both allows, with a byte tail
XM_IGROUPS_FN bool indelLettersEqual(const char* a, const char* b, long long n) {
  long long at = 0;
  const int piece = indelPiece(a, b);
  if (piece == 8) {
    for (; at + 8 <= n; at += 8) if (*(const unsigned long long*)(a + at) != *(const unsigned long long*)(b + at)) return false;
  } else if (piece == 4) {
    for (; at + 4 <= n; at += 4) if (*(const uint32_t*)(a + at) != *(const uint32_t*)(b + at)) return false;
  }
  for (; at < n; at++) if (a[at] != b[at]) return false;
  return true;
}
// to[0 .. n) = from[0 .. n), in the same pieces
XM_IGROUPS_FN void indelLettersCopy(char* to, const char* from, long long n) {
  long long at = 0;
  const int piece = indelPiece(to, from);
  if (piece == 8) {
    for (; at + 8 <= n; at += 8) *(unsigned long long*)(to + at) = *(const unsigned long long*)(from + at);
  } else if (piece == 4) {
    for (; at + 4 <= n; at += 4) *(uint32_t*)(to + at) = *(const uint32_t*)(from + at);
  }
  for (; at < n; at++) to[at] = from[at];
}

// the item's key is the group's (arena: where the groups' letters lie)
XM_IGROUPS_FN bool indelSameKey(const IndelGroup& g, const char* arena, const IndelItem& it) {
  if (g.contig != it.contig || g.kind != it.kind || g.pos1 != it.pos1 || g.length != it.length || g.numLetters != it.numLetters) return false;
  return indelLettersEqual(arena + g.lettersAt, it.letters, it.numLetters);
}

// the bytes a group's letters take in the arena: every group's letters start on an 8-byte boundary
XM_IGROUPS_FN long long indelArenaBytes(long long numLetters) { return (numLetters + 7) & ~7ll; }

// ---------------------------------------------------------------- the table's words
// keys[cap]: the fingerprint of the slot, 0 = empty.  words[cap]: XM_IGROUPS_NONE = no group and nobody asked; below XM_IGROUPS_REP = the index of the slot's
// group; XM_IGROUPS_REP | i = item i of the running call is the slot's representative and will make its group (the lowest such i: one atomic min, which leaves
// a group's index alone).  A call ends with every word it touched holding a group's index, so nothing the size of the table is ever reset.
constexpr unsigned long long XM_IGROUPS_NONE = ~0ull;
constexpr unsigned long long XM_IGROUPS_REP = 1ull << 62;

// the first slot a fingerprint probes (cap a power of two)
XM_IGROUPS_FN unsigned long long indelFirstSlot(unsigned long long fingerprint, unsigned long long mask) { return fingerprint & mask; }

// The capacity a table needs for `groups` groups and `n` more items: a power of two, at most half full.
XM_IGROUPS_FN unsigned long long indelCapacityFor(unsigned long long groups, unsigned long long n, unsigned long long least) {
  unsigned long long cap = least < 4 ? 4 : least;
  while (cap & (cap - 1)) cap += cap & (~cap + 1);  // (up to a power of two)
  while (cap < 2 * (groups + n)) cap <<= 1;
  return cap;
}

}  // namespace xm
