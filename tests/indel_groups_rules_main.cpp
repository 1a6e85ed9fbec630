// TEST INFRASTRUCTURE ONLY.  A sequential restatement of the fold of mapper_amd/csrc/xm_indel_groups.h over the plain rules of xm_indel_groups_rules.h - the
// very functions the kernels call - for tests/test_indel_groups_rules.py: claim (probe, the lowest item of a slot without a group is its representative), place
// (a record and the letters in the arena, in item order), add (the key compared with the slot's group, letters included: equal - the weight is added;
// different - left over), and the growth of the table, the records and the arena before each call.  After every growth of the table every group is looked up
// again through its fingerprint.
//
// usage: indel_groups_rules_main <case file>
//   bits <fingerprint bits>
//   capacity <initial capacity>
//   calls <k>
//   then per call: events <n>, and per event a line of its eight words and its letters ("-" for none)
// output: one line "group contig kind pos1 length support letters" per group, "left call <the eight words> letters" per left-over event in call order,
// and "grows <table> <records> <arena>", "found <groups looked up after growths>".
#include "../mapper_amd/csrc/xm_indel_groups_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

struct Event {
  long long w[8];
  std::string text;
};

struct Table {
  std::vector<unsigned long long> keys, words;
  std::vector<xm::IndelGroup> groups;   // (capacity: groups.size(); in use: count)
  std::vector<char> arena;
  long long count = 0, arenaUsed = 0;
  long long tableGrows = 0, recordGrows = 0, arenaGrows = 0, found = 0;
  int bits = 64;
  unsigned long long least = 4;
};

[[noreturn]] void die(const std::string& why) {
  std::cerr << "indel_groups_rules_main: " << why << "\n";
  std::exit(2);
}

unsigned long long probe(const Table& t, unsigned long long h) {
  const unsigned long long mask = t.keys.size() - 1;
  unsigned long long at = xm::indelFirstSlot(h, mask);
  while (t.keys[at] != 0 && t.keys[at] != h) at = (at + 1) & mask;
  return at;
}

void reserve(Table& t, long long n, long long textBytes) {
  const unsigned long long cap = t.keys.size();
  const unsigned long long want = xm::indelCapacityFor((unsigned long long)t.count, (unsigned long long)n, cap ? cap : t.least);
  if (want != cap) {
    Table bigger;
    bigger.keys.assign(want, 0ull);
    bigger.words.assign(want, xm::XM_IGROUPS_NONE);
    for (unsigned long long s = 0; s < cap; s++) {  // the re-insert: the fingerprints are distinct, there is nothing to compare
      if (t.keys[s] == 0) continue;
      const unsigned long long at = probe(bigger, t.keys[s]);
      if (bigger.keys[at] != 0) die("a fingerprint was in the old table twice");
      bigger.keys[at] = t.keys[s];
      bigger.words[at] = t.words[s];
    }
    t.keys.swap(bigger.keys);
    t.words.swap(bigger.words);
    if (cap) {
      t.tableGrows++;
      for (long long g = 0; g < t.count; g++) {  // every key is found again
        const xm::IndelItem it = xm::indelItemOfGroup(t.groups[(size_t)g], t.arena.data());
        const unsigned long long at = probe(t, xm::indelFingerprint(it, t.bits));
        if (t.keys[at] == 0 || t.words[at] != (unsigned long long)g) die("group " + std::to_string(g) + " is not found after the table grew");
        t.found++;
      }
    }
  }
  if ((long long)t.groups.size() < t.count + n) {
    if (!t.groups.empty()) t.recordGrows++;
    t.groups.resize((size_t)(t.count + n));
  }
  const long long letters = textBytes + 7 * n < 8 * textBytes ? textBytes + 7 * n : 8 * textBytes;
  if ((long long)t.arena.size() < t.arenaUsed + letters + 8) {
    if (!t.arena.empty()) t.arenaGrows++;
    t.arena.resize((size_t)(t.arenaUsed + letters + 8));
  }
}

// -> the indices of the items left over
std::vector<size_t> fold(Table& t, const std::vector<Event>& events) {
  const size_t n = events.size();
  std::vector<xm::IndelItem> items(n);
  std::vector<long long> slotOf(n, -1);
  for (size_t i = 0; i < n; i++) {  // claim
    items[i] = xm::indelItemOfEvent(events[i].w, events[i].text.data(), (long long)events[i].text.size());
    if (!xm::indelGrouped(events[i].w[5])) continue;
    const unsigned long long h = xm::indelFingerprint(items[i], t.bits);
    if (h == 0) die("a fingerprint of 0");
    const unsigned long long at = probe(t, h);
    t.keys[at] = h;
    const unsigned long long ask = xm::XM_IGROUPS_REP | (unsigned long long)i;
    if (ask < t.words[at]) t.words[at] = ask;
    slotOf[i] = (long long)at;
  }
  for (size_t i = 0; i < n; i++) {  // mark, scan and place: the representatives in item order
    if (slotOf[i] < 0 || t.words[(size_t)slotOf[i]] != (xm::XM_IGROUPS_REP | (unsigned long long)i)) continue;
    const xm::IndelItem& it = items[i];
    xm::IndelGroup g;
    g.contig = it.contig; g.kind = it.kind; g.pos1 = it.pos1; g.length = it.length; g.numLetters = it.numLetters; g.lettersAt = t.arenaUsed; g.support = 0;
    if (t.count >= (long long)t.groups.size() || t.arenaUsed + xm::indelArenaBytes(it.numLetters) > (long long)t.arena.size()) die("the table was not grown for the call");
    xm::indelLettersCopy(t.arena.data() + g.lettersAt, it.letters, it.numLetters);
    t.groups[(size_t)t.count] = g;
    t.words[(size_t)slotOf[i]] = (unsigned long long)t.count;
    t.count++;
    t.arenaUsed += xm::indelArenaBytes(it.numLetters);
  }
  std::vector<size_t> left;
  for (size_t i = 0; i < n; i++) {  // add
    if (slotOf[i] < 0) continue;
    const unsigned long long g = t.words[(size_t)slotOf[i]];
    if (g >= (unsigned long long)t.count) die("a slot without a group after place");
    if (xm::indelSameKey(t.groups[(size_t)g], t.arena.data(), items[i])) t.groups[(size_t)g].support += items[i].weight;
    else left.push_back(i);
  }
  return left;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: indel_groups_rules_main <case file>");
  std::ifstream in(argv[1]);
  if (!in) die("cannot read the case file");
  std::string word;
  Table t;
  long long bits = 64, capacity = 4, calls = 0;
  if (!(in >> word >> bits) || word != "bits") die("bits expected");
  if (!(in >> word >> capacity) || word != "capacity") die("capacity expected");
  if (!(in >> word >> calls) || word != "calls") die("calls expected");
  t.bits = (int)(bits > 64 ? 64 : bits);
  t.least = (unsigned long long)capacity;
  for (long long c = 0; c < calls; c++) {
    long long n = 0;
    if (!(in >> word >> n) || word != "events" || n < 0) die("events expected");
    std::vector<Event> events((size_t)n);
    long long textBytes = 0;
    for (Event& e : events) {
      for (long long& x : e.w) if (!(in >> x)) die("an event has eight words");
      if (!(in >> e.text)) die("an event has letters or -");
      if (e.text == "-") e.text.clear();
      textBytes += (long long)e.text.size();
    }
    if (n == 0) continue;
    reserve(t, n, textBytes);
    if (t.keys.size() < 2 * (size_t)(t.count + n) || (t.keys.size() & (t.keys.size() - 1))) die("the capacity is no power of two or the table more than half full");
    for (size_t i : fold(t, events)) {
      std::printf("left %lld", c);
      for (long long x : events[i].w) std::printf(" %lld", x);
      std::printf(" %s\n", events[i].text.empty() ? "-" : events[i].text.c_str());
    }
  }
  for (long long g = 0; g < t.count; g++) {
    const xm::IndelGroup& r = t.groups[(size_t)g];
    const std::string letters(t.arena.data() + r.lettersAt, (size_t)r.numLetters);
    std::printf("group %d %d %lld %lld %llu %s\n", r.contig, r.kind, (long long)r.pos1, (long long)r.length, r.support, letters.empty() ? "-" : letters.c_str());
  }
  std::printf("grows %lld %lld %lld\nfound %lld\n", t.tableGrows, t.recordGrows, t.arenaGrows, t.found);
  return 0;
}
