// Stand-alone driver of mapper_amd/csrc/xm_memo_plan.h for tests/test_memo_plan.py: the plan of a budget, and the memory's table run on the host with the
// very functions the kernels of xm_memo.h call (memoProbe, memoClaim, memoReserve, ...), one "launch" at a time as xm_capi.hip's memoLookup / memoInsert
// drive them.  Commands on stdin, one answer line per command on stdout:
//   plan <budget>                                   -> slots arenaBytes capacity tableBytes
//   record <len0> <len1> <intLen> <dblLen>          -> bytesAt intsAt dblsAt recordBytes
//   fp <hex fingerprint> <bits>                     -> hex
//   differ <filled> <hex bytes a> <hex bytes b>     -> 0 | 1            (memoMustEmpty)
//   new <budget> <bits>                             -> ok | refused
//   insert <k>, then k lines <hex fingerprint> <content id> <len0> <len1> <intLen> <dblLen>
//                                                   -> k answers (stored <offset> | dropped | dead | skipped), then "state <claimed> <cursor> <records> <used> <full>"
//   lookup <hex fingerprint> <content id> <len0> <len1>   -> record offset and its intLen dblLen, or -1
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

struct Memory {
  MemoPlan plan{0, 0, 0};
  int bits = 64;
  std::vector<unsigned long long> keys, offs;
  std::vector<uint8_t> arena;
  unsigned long long state[4] = {0, 0, 0, 0};  // claimed, cursor, records
  unsigned long long mask() const { return (unsigned long long)plan.slots - 1; }
  MemoHeader headerOf(const Item& it) const {
    MemoHeader h;
    memset(&h, 0, sizeof(h));
    h.mateCount = it.len1 > 0 ? 2 : 1; h.len0 = it.len0; h.len1 = it.len1; h.intLen = it.intLen; h.dblLen = it.dblLen;
    h.innerBits = it.content >> 7; h.deviationBits = it.content << 3;
    return h;
  }
  // xm_memo_insert_kernel, one item
  std::string insertOne(const Item& it) {
    const MemoHeader hd = headerOf(it);
    const unsigned long long h = memoFingerprint(it.fp, bits);
    const long long slot = memoClaim(keys.data(), mask(), h, [](unsigned long long* a, unsigned long long expected, unsigned long long desired) {
      const unsigned long long was = *a;
      if (was == expected) *a = desired;
      return was;
    });
    if (slot < 0) return "dropped";
    state[0]++;
    const unsigned long long at = memoReserve(&state[1], (unsigned long long)plan.arenaBytes, memoRecordBytes(hd), [](unsigned long long* a, unsigned long long k) {
      const unsigned long long was = *a;
      *a += k;
      return was;
    });
    if (at == XM_MEMO_DEAD) return "dead";
    state[2]++;
    uint8_t* rec = arena.data() + at;
    memcpy(rec, &hd, sizeof(hd));
    for (int i = 0; i < it.len0 + it.len1; i++) rec[memoBytesAt(hd) + i] = byteOf(it.content, i);
    for (int i = 0; i < it.intLen; i++) { const int32_t v = (int32_t)(it.content + (unsigned)i); memcpy(rec + memoIntsAt(hd) + 4 * (size_t)i, &v, 4); }
    for (int i = 0; i < it.dblLen; i++) { const double v = (double)it.content + i; memcpy(rec + memoDblsAt(hd) + 8 * (size_t)i, &v, 8); }
    offs[slot] = at;
    return "stored " + std::to_string(at);
  }
  // xm_memo_lookup_kernel, one query
  std::string lookupOne(const Item& it) const {
    const MemoHeader want = headerOf(it);
    const long long at = memoSlotRecord(offs.data(), memoProbe(keys.data(), mask(), memoFingerprint(it.fp, bits)));
    if (at < 0) return "-1";
    MemoHeader hd;
    memcpy(&hd, arena.data() + at, sizeof(hd));
    bool same = hd.mateCount == want.mateCount && hd.len0 == want.len0 && hd.len1 == want.len1 && hd.innerBits == want.innerBits && hd.deviationBits == want.deviationBits;
    for (int i = 0; same && i < hd.len0 + hd.len1; i++) same = arena[at + memoBytesAt(hd) + i] == byteOf(it.content, i);
    if (!same) return "-1";
    // the slices must be the ones stored for this content
    for (int i = 0; i < hd.intLen; i++) { int32_t v; memcpy(&v, arena.data() + at + memoIntsAt(hd) + 4 * (size_t)i, 4); if (v != (int32_t)(it.content + (unsigned)i)) return "corrupt"; }
    for (int i = 0; i < hd.dblLen; i++) { double v; memcpy(&v, arena.data() + at + memoDblsAt(hd) + 8 * (size_t)i, 8); if (v != (double)it.content + i) return "corrupt"; }
    return std::to_string(at) + " " + std::to_string(hd.intLen) + " " + std::to_string(hd.dblLen);
  }
};

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return b;
}

int main() {
  Memory m;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "plan") {
      long long budget;
      in >> budget;
      const MemoPlan p = memoPlan(budget);
      printf("%lld %lld %lld %lld\n", p.slots, p.arenaBytes, p.capacity, memoTableBytes(p));
    } else if (cmd == "record") {
      Item it{0, 0, 0, 0, 0, 0};
      in >> it.len0 >> it.len1 >> it.intLen >> it.dblLen;
      const MemoHeader h = m.headerOf(it);
      printf("%llu %llu %llu %llu\n", memoBytesAt(h), memoIntsAt(h), memoDblsAt(h), memoRecordBytes(h));
    } else if (cmd == "fp") {
      std::string hex; int bits;
      in >> hex >> bits;
      printf("%llx\n", memoFingerprint(strtoull(hex.c_str(), nullptr, 16), bits));
    } else if (cmd == "differ") {
      int filled; std::string a, b;
      in >> filled >> a >> b;
      const std::vector<uint8_t> x = unhex(a), y = unhex(b);
      printf("%d\n", x.size() == y.size() && memoMustEmpty(filled != 0, x.data(), y.data(), x.size()) ? 1 : 0);
    } else if (cmd == "new") {
      long long budget;
      in >> budget >> m.bits;
      m.plan = memoPlan(budget);
      if (m.plan.slots == 0) { printf("refused\n"); continue; }
      m.keys.assign((size_t)m.plan.slots, 0ull); m.offs.assign((size_t)m.plan.slots, XM_MEMO_DEAD); m.arena.assign((size_t)m.plan.arenaBytes, 0);
      m.state[0] = m.state[1] = m.state[2] = 0;
      printf("ok\n");
    } else if (cmd == "insert") {
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
      // memoInsert of xm_capi.hip: no launch into a full memory, and never more items than the table has room for
      long long n = k < memoRoom(m.plan, m.state[0]) ? k : memoRoom(m.plan, m.state[0]);
      if (memoFull(m.plan, m.state[0], m.state[1])) n = 0;
      for (long long i = 0; i < k; i++) printf("%s\n", i < n ? m.insertOne(items[(size_t)i]).c_str() : "skipped");
      printf("state %llu %llu %llu %llu %d\n", m.state[0], m.state[1], m.state[2], memoArenaUsed(m.plan, m.state[1]), memoFull(m.plan, m.state[0], m.state[1]) ? 1 : 0);
    } else if (cmd == "lookup") {
      Item it{0, 0, 0, 0, 0, 0};
      std::string hex;
      in >> hex >> it.content >> it.len0 >> it.len1;
      it.fp = strtoull(hex.c_str(), nullptr, 16);
      printf("%s\n", m.lookupOne(it).c_str());
    } else if (!cmd.empty()) {
      printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
