// The plan of an index build, as plain host C++: every decision the seed tables depend on that is arithmetic and not hashing.  The host builder
// (xm_index_host.h, hashLengths) and the GPU builder (xm_index_device.hip, deviceHashLengths) must give the same tables bit for bit; both take the
// knobs, the shape of a table, the cut into groups, a group's bucket layout, the sort keys and the placement of the tables from here, so neither
// holds a copy of its own.  No HIP, no threads, nothing of HostIndex but values passed in: tests/test_index_plan.py checks it without a GPU.
#pragma once
#include "xm_defs.h"
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <vector>

namespace xm {

// Every XM_* variable an index build reads, filled once per hashLengths call, which hands them to the GPU build (tests set them between the calls of one process).
struct BuildKnobs {
  bool deviceBuild;     // XM_DEVICE_BUILD (0: hash on the host even though a GPU is there)
  bool hybridOnHost;    // XM_BUILD_HYBRID_ON_HOST (test hook): on the host, the composition the GPU build uses for contigs with ambiguity codes
  bool threadsSet;      // XM_BUILD_THREADS: host threads of the build (unset or empty: the hardware's)
  int threads;
  int spliceMin;        // XM_BUILD_SPLICE_MIN (test hook): a run of N of this length or longer is not held whole in a window (2 048; at least 64)
  bool groupRecordsSet; // XM_BUILD_GROUP_RECORDS (testing: force several groups): records per group of tables (unset or empty: from the free memory)
  unsigned long long groupRecords;
  bool trace;           // XM_TRACE_BUILD (set at all: on)
};
inline BuildKnobs readBuildKnobs() {
  const auto value = [](const char* name) { const char* e = getenv(name); return (e && *e) ? e : nullptr; };  // (an empty value means unset)
  BuildKnobs k;
  const char* e = value("XM_DEVICE_BUILD");
  k.deviceBuild = !(e && atoi(e) == 0);
  e = value("XM_BUILD_HYBRID_ON_HOST");
  k.hybridOnHost = e && atoi(e) != 0;
  e = value("XM_BUILD_THREADS");
  k.threadsSet = e != nullptr;
  k.threads = e ? atoi(e) : 0;
  e = value("XM_BUILD_SPLICE_MIN");
  k.spliceMin = e ? (atoi(e) < 64 ? 64 : atoi(e)) : 2048;
  e = value("XM_BUILD_GROUP_RECORDS");
  k.groupRecordsSet = e != nullptr;
  k.groupRecords = e ? strtoull(e, nullptr, 10) : 0;
  k.trace = getenv("XM_TRACE_BUILD") != nullptr;
  return k;
}

// ---- the shape of a table
struct TableShape { int32_t capacity, maxCount; };  // buckets; maxInterestingCountPerKey
inline TableShape tableShape(long long estimatedCapacity, int L, int maxNumShortMatches) {
  long long cap = estimatedCapacity;
  if (cap < 1) cap = 1;
  if (cap > INT32_MAX / 2) cap = INT32_MAX / 2;  // M/PackedMap.java:22-25
  long long mx = (long long)L * L;  // M/HashBlock_Database.java:569-576
  if (mx < maxNumShortMatches) mx = maxNumShortMatches;
  if (mx > 32766) mx = 32766;
  if (mx < 1) mx = 1;
  return TableShape{(int32_t)cap, (int32_t)mx};
}
// a table that receives no record (and every table below minInterestingSize) is the reference's PackedMap(1, 1) placeholder (M/HashBlock_Database.java:387-393)
inline TableShape placeholderShape() { return TableShape{1, 1}; }
inline TableShape shapeFor(const TableShape& planned, unsigned long long nRecords) { return nRecords == 0 ? placeholderShape() : planned; }
// [maxLen + 1]: the shapes of the tables [lo, maxLen] (zeros below lo: those tables receive no record); estimate(L) = HostIndex::estimateRequiredCapacity
template <typename Estimate>
inline std::vector<TableShape> tableShapes(int lo, int maxLen, int maxNumShortMatches, Estimate&& estimate) {
  std::vector<TableShape> shapes((size_t)maxLen + 1, TableShape{0, 0});
  for (int L = lo; L <= maxLen; L++) shapes[(size_t)L] = tableShape(estimate(L), L, maxNumShortMatches);
  return shapes;
}
inline std::vector<int> capacitiesOf(const std::vector<TableShape>& shapes) {  // (what the hashing takes a record's bucket from)
  std::vector<int> c(shapes.size());
  for (size_t L = 0; L < shapes.size(); L++) c[L] = shapes[L].capacity;
  return c;
}

// ---- groups of consecutive tables whose records fit a budget (GPU build: a sort needs both record arrays twice + its own scratch, 40 bytes a record in
// half of the free memory)
inline unsigned long long recordBudget(size_t freeBytes) { return (unsigned long long)(freeBytes / 2) / 40; }
struct TableGroup { int gLo, gHi; unsigned long long nRecs; };
// greedy: a table joins the group while the group's records stay within the budget (at least 1); a table that alone exceeds it is a group on its own
inline std::vector<TableGroup> planGroups(const std::vector<unsigned long long>& hist, int minLen, int maxLen, unsigned long long budgetRecs) {
  if (budgetRecs < 1) budgetRecs = 1;
  std::vector<TableGroup> groups;
  for (int gLo = minLen; gLo <= maxLen;) {
    TableGroup g{gLo, gLo, hist[(size_t)gLo]};
    while (g.gHi + 1 <= maxLen && g.nRecs + hist[(size_t)(g.gHi + 1)] <= budgetRecs) { g.gHi++; g.nRecs += hist[(size_t)g.gHi]; }
    groups.push_back(g);
    gLo = g.gHi + 1;
  }
  return groups;
}

// a group's tables side by side: bucketBase = first of the table's capacity + 1 offset entries in the group
struct TableDesc { unsigned long long bucketBase; int32_t capacity, maxCount; };
struct GroupLayout { std::vector<TableDesc> tables; unsigned long long nEntries; };
inline GroupLayout layoutGroup(const TableGroup& g, const std::vector<unsigned long long>& hist, const std::vector<TableShape>& shapes) {
  GroupLayout lay;
  lay.tables.resize((size_t)(g.gHi - g.gLo + 1));
  lay.nEntries = 0;
  for (int L = g.gLo; L <= g.gHi; L++) {
    const TableShape s = shapeFor(shapes[(size_t)L], hist[(size_t)L]);
    lay.tables[(size_t)(L - g.gLo)] = TableDesc{lay.nEntries, s.capacity, s.maxCount};
    lay.nEntries += (unsigned long long)s.capacity + 1;
  }
  return lay;
}

// ---- the order of a table's records: (bucket, position, single before multi).  A record's position word carries "comes from a possibility of a multi
// block" in its top bit; the word that sorts is the position shifted left by one with that flag in bit 0.
constexpr uint64_t XM_REC_MULTI = 1ull << 63;
inline uint64_t sortPosWord(uint64_t pos) { return (pos << 1) | (pos >> 63); }
// GPU build: a record's key is (table within its group, bucket)
inline unsigned long long sortKeyWord(int tableInGroup, uint32_t bucket) { return ((unsigned long long)(unsigned)tableInGroup << 32) | bucket; }
// bits the two stable radix sorts of the GPU build look at: the position word (lastCumStart = the end of the encoded positions; one more bit with the
// multi flag) and, above the 32 bits of the bucket, the table
struct SortKeyBits { unsigned posBits, tableBits; };
inline SortKeyBits sortKeyBits(unsigned long long lastCumStart, bool ambiguous, int nTables) {
  SortKeyBits b{1, 1};
  while (b.posBits < 64 && (lastCumStart >> b.posBits) != 0) b.posBits++;
  if (ambiguous) b.posBits++;  // (positions are shifted left by one, bit 0 = multi: single before multi at the same position)
  while ((1 << b.tableBits) < nTables) b.tableBits++;
  return b;
}

// ---- appending tables to the host index.  stored[k] = positions table firstL + k stores; the tables' offset entries (capacity + 1 each) start at offBase
// of bucketOff, their positions at posBase of positions, one table behind the other.
inline unsigned long long storedTotal(const std::vector<unsigned long long>& stored) {
  unsigned long long total = 0;
  for (unsigned long long s : stored) {
    if (s > 0x7FFFFFFFull) throw std::runtime_error("table too large for 31-bit bucket offsets");  // (bit 31 of an offset entry is XM_OVERFULL)
    total += s;
  }
  return total;
}
inline void placeTables(std::vector<Table>& tables, int firstL, const std::vector<TableDesc>& desc, const std::vector<unsigned long long>& stored, size_t offBase, size_t posBase) {
  unsigned long long posAt = 0;
  for (size_t k = 0; k < desc.size(); k++) {
    Table t;
    t.capacity = desc[k].capacity; t.maxCount = desc[k].maxCount;
    t.offBase = (int64_t)(offBase + (size_t)desc[k].bucketBase);
    t.posBase = (int64_t)(posBase + (size_t)posAt);
    posAt += stored[k];
    tables[(size_t)firstL + k] = t;
  }
}

}  // namespace xm
