// The rules of the mutations file run on the host (tests/test_mutations_rules.py): a stand-alone program over mapper_amd/csrc/xm_mutations_rules.h, the header
// the kernels of xm_mutations.h call on the device.  It reads a case - words separated by blanks:
//   filter <minSNPTotal> <minIndelStartTotal> <minIndelContinuationTotal> <SNP fraction> <start fraction> <continuation fraction>
//   contigs <n> <length> ...
//   counts <total>, then total depths, 4 * total alts (plane by plane) and total middle depths, in units
//   candidates <k>, then k times <contig> <kind> <pos1> <length> <support units>
// and prints "snp <contig> <0-based position> <letter> <support units> <total units>" for every row in position-then-letter order, walking all forward
// positions as the select kernels do (the contig by mutationsContigOf), then "verdict <total units> <keep>" per candidate.
#include "../mapper_amd/csrc/xm_mutations_rules.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static void bad(const std::string& what) {
  std::fprintf(stderr, "mutations_rules_main: %s\n", what.c_str());
  std::exit(2);
}

int main(int argc, char** argv) {
  if (argc != 2) bad("usage: mutations_rules_main <case file>");
  std::ifstream in(argv[1]);
  if (!in) bad("cannot open the case");
  std::string word;
  xm::MutationFilter f{};
  double fractions[3];
  if (!(in >> word) || word != "filter") bad("filter expected");
  if (!(in >> f.minSNPTotalDepth >> f.minIndelTotalStartDepth >> f.minIndelContinuationTotalDepth >> fractions[0] >> fractions[1] >> fractions[2])) bad("six thresholds expected");
  f.minSNPDepthFraction = (float)fractions[0]; f.minIndelStartDepthFraction = (float)fractions[1]; f.minIndelContinuationDepthFraction = (float)fractions[2];
  int numContigs = 0;
  if (!(in >> word >> numContigs) || word != "contigs" || numContigs < 1) bad("contigs expected");
  std::vector<int64_t> start((size_t)numContigs);
  std::vector<long long> length((size_t)numContigs);
  long long total = 0;
  for (int c = 0; c < numContigs; c++) {
    if (!(in >> length[(size_t)c]) || length[(size_t)c] < 1) bad("a contig length >= 1 expected");
    start[(size_t)c] = total;
    total += length[(size_t)c];
  }
  long long given = 0;
  if (!(in >> word >> given) || word != "counts" || given != total) bad("counts <total> expected");
  std::vector<unsigned long long> depth((size_t)total), alt((size_t)total * 4), middle((size_t)total);
  for (auto& x : depth) if (!(in >> x)) bad("depth");
  for (auto& x : alt) if (!(in >> x)) bad("alt");
  for (auto& x : middle) if (!(in >> x)) bad("middle");
  long long k = 0;
  if (!(in >> word >> k) || word != "candidates" || k < 0) bad("candidates expected");
  struct Candidate { int contig, kind; long long pos1, n; unsigned long long support; };
  std::vector<Candidate> candidates((size_t)k);
  for (auto& c : candidates) {
    if (!(in >> c.contig >> c.kind >> c.pos1 >> c.n >> c.support)) bad("a candidate's five fields expected");
    if (c.contig < 0 || c.contig >= numContigs || (c.kind != 1 && c.kind != 2)) bad("a candidate outside of the reference");
  }
  for (long long pos = 0; pos < total; pos++)
    for (int b = 0; b < 4; b++) {
      const unsigned long long a = alt[(size_t)b * (size_t)total + (size_t)pos];
      if (!xm::mutationsSnpRow(a, depth[(size_t)pos], f)) continue;
      const int contig = xm::mutationsContigOf(start.data(), numContigs, pos);
      std::cout << "snp " << contig << " " << pos - start[(size_t)contig] << " " << b << " " << a << " " << depth[(size_t)pos] << "\n";
    }
  for (const auto& c : candidates) {
    unsigned long long units = 0;
    const long long keep = xm::mutationsJudgeIndel(middle.data() + start[(size_t)c.contig], length[(size_t)c.contig], c.pos1, c.kind, c.n, c.support, f, &units);
    std::cout << "verdict " << units << " " << keep << "\n";
  }
  return 0;
}
