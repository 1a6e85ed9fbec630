// libxm_hostio.so: host-side I/O of the standalone harness (`python -m mapper_amd`) in native code - FASTA / FASTQ (plain or .gz) into the flat
// batch arrays of include/xmapper_hip.h without one object per read, and the result streams of a batch into SAM text (and the unaligned-query file) without
// one object per alignment.  SURVEY.md section 8(f) rank 1: the harness around the accelerated path.  In the drop-in deployment the Java host keeps doing
// all of this (north_star: "all I/O stays Java"): Mapper.java:699-732 hands QueryAlignments to its SamWriter; this library is what lets the Python harness
// feed a kernel that aligns millions of reads per second.  Plain C++17 for the host, no GPU code, no part of the alignment path.
//
// What the reference pins of the formats: the five SAM bodies of SamWriter_Test.java:18-94 (flags 0 / 99 / 147 / 73, MAPQ 255, column 9 = read length, RNEXT =
// contig name, mate 2 printed as aligned, `cs:f:` only for paired queries, `AS:f:` = Double.toString of the penalty), the section rule of
// SequenceSplitter.java:9-38, the statistics of Mapper.run :786-796.  What they do not show follows the SAM specification and is marked [unpinned] in
// mapper_amd/sam.py, whose records() this formatter reproduces byte for byte (tests/test_hostio.py compares the two on random result streams).
#include "../../include/xmapper_hostio.h"
#include "../csrc/xm_fastq_rules.h"
#include "../csrc/xm_fasta_rules.h"
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <charconv>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>
#include <fcntl.h>
#include <sys/stat.h>

namespace {

thread_local std::string g_error;
int fail(const std::string& m) { g_error = m; return -1; }

uint8_t g_code[256];
uint8_t g_comp[16];
const char g_decode[17] = "?ACMGRSVTWYHKDBN";
struct Tables {
  Tables() {
    memset(g_code, 15, sizeof(g_code));
    const char* letters = "ACGTURYSWKMBDHVN";
    const uint8_t values[16] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    for (int i = 0; i < 16; i++) { g_code[(uint8_t)letters[i]] = values[i]; g_code[(uint8_t)(letters[i] | 0x20)] = values[i]; }
    for (int b = 0; b < 16; b++) g_comp[b] = (uint8_t)(((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3));
  }
} g_tables;

// ---------------------------------------------------------------- reading
struct Source {
  gzFile f = nullptr;
  std::string path;
  std::vector<char> buf;
  size_t pos = 0, end = 0;
  bool eof = false;
  long long line = 0;
  int fd = -1;  // an uncompressed file is read directly (zlib's transparent mode would copy every byte once more)
  bool open(const char* p) {
    path = p;
    buf.resize(8 << 20);
    FILE* probe = fopen(p, "rb");
    if (!probe) return false;
    unsigned char magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, probe);
    fclose(probe);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
      f = gzopen(p, "rb");
      if (!f) return false;
      gzbuffer(f, 1 << 20);
    } else {
      fd = ::open(p, O_RDONLY);
      if (fd < 0) return false;
    }
    return true;
  }
  void close() { if (f) gzclose(f); f = nullptr; if (fd >= 0) ::close(fd); fd = -1; }
  bool fill(size_t most = 1u << 30) {  // keeps [pos, end), reads more behind it (at most `most` bytes)
    if (eof) return false;
    if (pos > 0) { memmove(buf.data(), buf.data() + pos, end - pos); end -= pos; pos = 0; }
    if (end == buf.size()) buf.resize(buf.size() * 2);
    const size_t room = std::min<size_t>(buf.size() - end, most);
    long n = f ? (long)gzread(f, buf.data() + end, (unsigned)room) : (long)::read(fd, buf.data() + end, room);
    if (n <= 0) { eof = true; return false; }
    end += (size_t)n;
    return true;
  }
  // next line without its terminator (\n or \r\n); false at end of input.  The view stays valid until the next call.
  bool getline(const char*& s, size_t& n) {
    while (true) {
      const char* nl = (const char*)memchr(buf.data() + pos, '\n', end - pos);
      if (nl) {
        s = buf.data() + pos;
        n = (size_t)(nl - s);
        pos += n + 1;
        if (n > 0 && s[n - 1] == '\r') n--;
        line++;
        return true;
      }
      if (!fill()) {
        if (pos < end) { s = buf.data() + pos; n = end - pos; pos = end; if (n > 0 && s[n - 1] == '\r') n--; line++; return true; }
        return false;
      }
    }
  }
  int peek() {  // first byte of the next line, -1 at end of input
    while (pos >= end) if (!fill()) return -1;
    return (unsigned char)buf[pos];
  }
};

struct Record { std::string name, seq, qual; bool hasQual = false; };

void trim(const char*& s, size_t& n) {
  while (n > 0 && (s[0] == ' ' || s[0] == '\t')) { s++; n--; }
  while (n > 0 && (s[n - 1] == ' ' || s[n - 1] == '\t' || s[n - 1] == '\r')) n--;
}

// one FASTA or FASTQ record (cli.read_sequences: the name is the header up to the first blank; FASTA sequences may span lines; a FASTQ record is four lines)
int nextRecord(Source& src, Record& r) {
  const char* s; size_t n;
  while (true) {
    if (!src.getline(s, n)) return 1;
    if (n > 0) break;
  }
  if (s[0] != '>' && s[0] != '@') return fail(src.path + ": line " + std::to_string(src.line) + " is neither a FASTA nor a FASTQ header");
  const bool fastq = s[0] == '@';
  size_t k = 1;
  while (k < n && s[k] != ' ' && s[k] != '\t') k++;
  r.name.assign(s + 1, k - 1);
  r.seq.clear(); r.qual.clear(); r.hasQual = false;
  if (fastq) {
    if (!src.getline(s, n)) return fail(src.path + ": FASTQ record without a sequence line at line " + std::to_string(src.line));
    trim(s, n);
    r.seq.assign(s, n);
    if (src.getline(s, n)) {  // '+'
      if (src.getline(s, n)) { trim(s, n); r.qual.assign(s, n); }
    }
    r.hasQual = true;
  } else {
    while (true) {
      const int c = src.peek();
      if (c < 0 || c == '>') break;
      src.getline(s, n);
      trim(s, n);
      r.seq.append(s, n);
    }
  }
  return 0;
}

}  // namespace

struct xmio_reader {
  Source a, b;
  bool paired = false;
  int split = 0;
  bool keepQual = false;
  // a record that was read and split into sections, of which the current batch took only some
  std::vector<std::pair<int, int>> pendingSections;
  size_t pendingNext = 0;
  Record pending;
};

struct BatchStore {
  std::vector<int32_t> mateCount, mateLength;
  std::vector<int64_t> mateOffset, nameOff, qualOff;
  std::vector<uint8_t> codes;
  std::string names, quals;
  std::vector<uint8_t> hasQual;
};

extern "C" {

const char* xmio_last_error(void) { return g_error.c_str(); }

xmio_reader* xmio_open(const char* path1, const char* path2, int32_t split_past_size, int32_t keep_qualities) {
  xmio_reader* r = new xmio_reader();
  if (!path1 || !r->a.open(path1)) { g_error = std::string("cannot open ") + (path1 ? path1 : "(null)"); delete r; return nullptr; }
  if (path2) {
    if (!r->b.open(path2)) { g_error = std::string("cannot open ") + path2; r->a.close(); delete r; return nullptr; }
    r->paired = true;
  }
  r->split = split_past_size;
  r->keepQual = keep_qualities != 0;
  return r;
}

void xmio_close(xmio_reader* r) {
  if (!r) return;
  r->a.close(); r->b.close();
  delete r;
}

void xmio_batch_free(xmio_batch* b) {
  if (!b) return;
  delete (BatchStore*)b->store;
  delete b;
}

// Up to max_queries queries (a pair is one query) into a new batch; *out = null at end of input.
int xmio_next(xmio_reader* r, int64_t max_queries, xmio_batch** out) {
  *out = nullptr;
  BatchStore* st = new BatchStore();
  auto addMate = [&](const std::string& name, const char* seq, size_t n, const std::string* qual) {
    st->mateOffset.push_back((int64_t)st->codes.size());
    st->mateLength.push_back((int32_t)n);
    const size_t at = st->codes.size();
    st->codes.resize(at + n);
    for (size_t i = 0; i < n; i++) st->codes[at + i] = g_code[(uint8_t)seq[i]];
    st->nameOff.push_back((int64_t)st->names.size());
    st->names += name;
    if (r->keepQual) {
      st->qualOff.push_back((int64_t)st->quals.size());
      st->hasQual.push_back(qual ? 1 : 0);
      if (qual) st->quals += *qual;
    }
  };
  auto padMate = [&]() {  // the unused second mate of a single query
    st->mateOffset.push_back(0); st->mateLength.push_back(0);
    st->nameOff.push_back((int64_t)st->names.size());
    if (r->keepQual) { st->qualOff.push_back((int64_t)st->quals.size()); st->hasQual.push_back(0); }
  };
  int64_t nq = 0;
  Record ra, rb;
  st->codes.reserve((size_t)std::min<int64_t>(max_queries, 1 << 20) * 160);
  // one mate straight from the file buffer into the batch (the common case: no sections); 0 = added, 1 = end of input, -1 = error
  auto directMate = [&](Source& src) -> int {
    const char* s; size_t n;
    while (true) {
      if (!src.getline(s, n)) return 1;
      if (n > 0) break;
    }
    if (s[0] != '>' && s[0] != '@') return fail(src.path + ": line " + std::to_string(src.line) + " is neither a FASTA nor a FASTQ header");
    const bool fastq = s[0] == '@';
    size_t k = 1;
    while (k < n && s[k] != ' ' && s[k] != '\t') k++;
    st->nameOff.push_back((int64_t)st->names.size());
    st->names.append(s + 1, k - 1);
    const size_t at = st->codes.size();
    st->mateOffset.push_back((int64_t)at);
    auto addBases = [&](const char* p, size_t m) {
      const size_t a0 = st->codes.size();
      st->codes.resize(a0 + m);
      uint8_t* c = st->codes.data() + a0;
      for (size_t i = 0; i < m; i++) c[i] = g_code[(uint8_t)p[i]];
    };
    if (fastq) {
      if (!src.getline(s, n)) return fail(src.path + ": FASTQ record without a sequence line at line " + std::to_string(src.line));
      trim(s, n);
      addBases(s, n);
      bool haveQual = false;
      if (src.getline(s, n) && src.getline(s, n)) { trim(s, n); haveQual = true; }
      if (r->keepQual) {
        st->qualOff.push_back((int64_t)st->quals.size());
        st->hasQual.push_back(1);
        if (haveQual) st->quals.append(s, n);
      }
    } else {
      while (true) {
        const int c = src.peek();
        if (c < 0 || c == '>') break;
        src.getline(s, n);
        trim(s, n);
        addBases(s, n);
      }
      if (r->keepQual) { st->qualOff.push_back((int64_t)st->quals.size()); st->hasQual.push_back(0); }
    }
    st->mateLength.push_back((int32_t)(st->codes.size() - at));
    return 0;
  };
  while (r->split <= 0 && nq < max_queries) {
    int rc = directMate(r->a);
    if (rc < 0) { delete st; return -1; }
    if (r->paired) {
      int rc2 = rc == 1 ? nextRecord(r->b, rb) : directMate(r->b);   // (at the end of the first file the second must end too)
      if (rc2 < 0) { delete st; return -1; }
      if (rc != rc2) { delete st; return fail("paired query files have different numbers of reads: " + r->a.path + ", " + r->b.path); }
    }
    if (rc == 1) break;
    if (!r->paired) padMate();
    st->mateCount.push_back(r->paired ? 2 : 1);
    nq++;
  }
  while (r->split > 0 && nq < max_queries) {
    if (r->pendingNext < r->pendingSections.size()) {  // sections of a long read left over from the previous batch
      const auto se = r->pendingSections[r->pendingNext++];
      addMate(r->pending.name, r->pending.seq.data() + se.first, (size_t)(se.second - se.first), nullptr);
      padMate();
      st->mateCount.push_back(1);
      nq++;
      continue;
    }
    int rc = nextRecord(r->a, ra);
    if (rc < 0) { delete st; return -1; }
    if (r->paired) {
      int rc2 = nextRecord(r->b, rb);
      if (rc2 < 0) { delete st; return -1; }
      if (rc != rc2) { delete st; return fail("paired query files have different numbers of reads: " + r->a.path + ", " + r->b.path); }
    }
    if (rc == 1) break;
    if (r->paired) {
      addMate(ra.name, ra.seq.data(), ra.seq.size(), ra.hasQual ? &ra.qual : nullptr);
      addMate(rb.name, rb.seq.data(), rb.seq.size(), rb.hasQual ? &rb.qual : nullptr);
      st->mateCount.push_back(2);
      nq++;
    } else if (r->split > 0) {
      // SequenceSplitter.java:9-38: (length - 1) / max + 1 sections, section k = [length * k / n, length * (k + 1) / n) in 64-bit integers; the sections carry no quality
      const long long length = (long long)ra.seq.size();
      const long long num = length > 0 ? (length - 1) / r->split + 1 : 1;
      r->pendingSections.clear();
      for (long long k = 0; k < num; k++) r->pendingSections.push_back(std::make_pair((int)(length * k / num), (int)(length * (k + 1) / num)));
      r->pendingNext = 0;
      r->pending = ra;
    } else {
      addMate(ra.name, ra.seq.data(), ra.seq.size(), ra.hasQual ? &ra.qual : nullptr);
      padMate();
      st->mateCount.push_back(1);
      nq++;
    }
  }
  if (nq == 0) { delete st; return 0; }
  st->nameOff.push_back((int64_t)st->names.size());
  if (r->keepQual) st->qualOff.push_back((int64_t)st->quals.size());
  if (st->codes.empty()) st->codes.push_back(0);
  xmio_batch* b = new xmio_batch();
  b->store = st;
  b->num_queries = nq;
  b->mate_count = st->mateCount.data(); b->mate_offset = st->mateOffset.data(); b->mate_length = st->mateLength.data();
  b->codes = st->codes.data(); b->codes_length = (int64_t)st->codes.size();
  b->names = st->names.data(); b->name_off = st->nameOff.data();
  b->quals = r->keepQual ? st->quals.data() : nullptr; b->qual_off = r->keepQual ? st->qualOff.data() : nullptr; b->has_qual = r->keepQual ? st->hasQual.data() : nullptr;
  *out = b;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- cutting (text blocks for the device parsers: the rules are ../csrc/xm_fastq_rules.h for four-line
// FASTQ records - scanBlock - and ../csrc/xm_fasta_rules.h for FASTA records of any number of lines - scanFastaBlock; multi-line FASTQ stays with xmio_open)
namespace {

constexpr int64_t kTextBlockLimit = 1ll << 30;  // bytes of one file in one block
constexpr size_t kTextFillBytes = 4u << 20;     // what the cutter reads at a time
constexpr size_t kTextBufferBytes = 8u << 20;   // the smallest buffer of a source (Source::open)

// The buffers the blocks' texts live in go round: a block of most of a source's buffer takes the buffer itself instead of a copy, the source goes on
// in another one, and a freed block's buffer waits here for the next source that needs one (its pages are mapped: no faults on the way).
std::mutex g_bufferMu;
std::vector<std::vector<char>> g_buffers;
std::vector<char> takeBuffer(size_t atLeast) {
  {
    std::lock_guard<std::mutex> lock(g_bufferMu);
    for (size_t i = 0; i < g_buffers.size(); i++)
      if (g_buffers[i].size() >= atLeast) { std::vector<char> b; b.swap(g_buffers[i]); g_buffers.erase(g_buffers.begin() + (long)i); return b; }
  }
  return std::vector<char>(std::max(atLeast, kTextBufferBytes));
}
void giveBuffer(std::vector<char>& b) {
  if (b.size() < kTextBufferBytes) return;
  std::lock_guard<std::mutex> lock(g_bufferMu);
  size_t held = b.size();
  for (const auto& x : g_buffers) held += x.size();
  if (g_buffers.size() < 4 && held <= ((size_t)2 << 30)) { g_buffers.emplace_back(); g_buffers.back().swap(b); }  // (at most four, and 2 GiB, wait)
}

// What the next block takes of a source: found without taking anything (the pair's other file may allow fewer records, then this is done again).
struct Cut {
  int64_t records = 0, bytes = 0, longest = 0;
  int64_t sections = 0;  // the queries the records give: `records`, or with a split size the sections of their sequence lines (xm::fastqLineSections)
  int64_t lines = 0;    // FASTA text (scanFastaBlock): the lines of the records; FASTQ text has four a record
  size_t consume = 0;   // bytes the source gives up: `bytes`, and at the end of the input the empty lines behind them
  bool atEnd = false;   // the source ended within this scan
};

// A full buffer grows at once to what the block will need, as far as the records so far (`bytes` of text) and the rest of a plain file tell (else fill()
// doubles it, and every doubling copies what is there).
void growAhead(Source& src, int64_t records, int64_t bytes, int64_t maxRecords) {
  if (src.pos != 0 || src.end != src.buf.size() || records < 256 || src.fd < 0) return;
  struct stat st;
  const off_t at = lseek(src.fd, 0, SEEK_CUR);
  if (fstat(src.fd, &st) != 0 || at < 0) return;
  const double perRecord = (double)bytes / (double)records;
  size_t want = (size_t)std::min<double>(perRecord * 1.125 * (double)maxRecords, (double)kTextBlockLimit) + 2 * kTextFillBytes;
  want = std::min<size_t>(want, src.end + (size_t)std::max<off_t>(st.st_size - at, 0) + kTextFillBytes);
  if (want > 2 * src.buf.size()) src.buf.resize(want);
}

// Whole records from src.pos on: line ends are found with memchr, every fourth ends a record.  Records of nothing but empty lines at the end of the
// block are left for the next one, which drops them if the input ends there.  false: the file ends inside a record, or a record is larger than a block.
// split > 0: maxRecords counts sections; the block stops in front of the record that would pass it, but takes at least one record with text.
bool scanBlock(Source& src, int64_t maxRecords, Cut& c, int64_t split = 0) {
  c = Cut();
  size_t off = 0, lineAt[4] = {0, 0, 0, 0}, lineTo[4] = {0, 0, 0, 0};  // (relative to src.pos: fill() moves the buffer)
  int inRecord = 0;  // complete lines of the record in progress
  bool someText = false;
  int64_t records = 0, bytes = 0, longest = 0, fullRecords = 0, fullBytes = 0;  // all records so far | up to the last one that is more than empty lines
  int64_t bytesAtMax = 0;
  int64_t sections = 0, fullSections = 0;  // (without a split size: the records)
  while (sections < maxRecords || fullRecords == 0) {  // (records of nothing but empty lines: on to the text behind them, or to the end, where they are dropped)
    const char* base = src.buf.data() + src.pos;
    const size_t avail = src.end - src.pos;
    const char* nl = off < avail ? (const char*)memchr(base + off, '\n', avail - off) : nullptr;
    if (!nl) {
      growAhead(src, records, bytes, maxRecords);
      if (!src.fill(kTextFillBytes)) { c.atEnd = true; break; }  // (a few MiB at a time: the lines are looked for while they are in the cache)
      continue;
    }
    const size_t e = (size_t)(nl - base);
    lineAt[inRecord] = off; lineTo[inRecord] = e;
    if (!xm::fastqEmptyLine(base, (long long)off, (long long)e)) someText = true;
    off = e + 1;
    if (++inRecord < 4) continue;
    if ((int64_t)off > kTextBlockLimit) {
      if (records > 0) break;  // the block is full
      g_error = src.path + ": a FASTQ record of more than 1 GiB at line " + std::to_string(src.line + 1);
      return false;
    }
    const int64_t ns = split > 0 ? (int64_t)xm::fastqLineSections(base, (long long)lineAt[1], (long long)lineTo[1], (long long)split) : 1;
    if (split > 0 && fullRecords > 0 && sections + ns > maxRecords) break;  // (the record stays for the next block)
    records++; bytes = (int64_t)off; sections += ns;
    if (records == maxRecords) bytesAtMax = bytes;
    longest = std::max(longest, (int64_t)(lineTo[1] - lineAt[1]));
    if (someText) { fullRecords = records; fullBytes = bytes; fullSections = sections; }
    inRecord = 0; someText = false;
  }
  if (c.atEnd) {
    const char* base = src.buf.data() + src.pos;
    const size_t avail = src.end - src.pos;
    int n = inRecord;
    if (inRecord < 4 && off < avail) { lineAt[n] = off; lineTo[n] = avail; n++; }  // a last line without its newline
    while (n > 0 && xm::fastqEmptyLine(base, (long long)lineAt[n - 1], (long long)lineTo[n - 1])) n--;  // trailing empty lines are dropped
    if (n == 4) {  // (three lines and the one without newline)
      const int64_t ns = split > 0 ? (int64_t)xm::fastqLineSections(base, (long long)lineAt[1], (long long)lineTo[1], (long long)split) : 1;
      if ((int64_t)avail > kTextBlockLimit && records > 0) { c.atEnd = false; }
      else if (split > 0 && fullRecords > 0 && sections + ns > maxRecords) { c.atEnd = false; }  // (the next block takes it)
      else {
        records++; bytes = (int64_t)avail; sections += ns; longest = std::max(longest, (int64_t)(lineTo[1] - lineAt[1]));
        fullRecords = records; fullBytes = bytes; fullSections = sections;
      }
    } else if (n > 0) {
      g_error = src.path + ": the file ends after " + std::to_string(n) + " of the 4 lines of a FASTQ record, at line " + std::to_string(src.line + 4 * records + n);
      return false;
    }
    if (split > 0) longest = std::min(longest, split);  // (an upper bound of the longest mate: no section is longer than the split size)
    if (c.atEnd) { c.records = fullRecords; c.bytes = fullBytes; c.sections = fullSections; c.longest = longest; c.consume = avail; return true; }
  }
  if (split == 0 && fullRecords > maxRecords) { fullRecords = fullSections = maxRecords; fullBytes = bytesAtMax; }  // (a block of empty lines with text behind them: the parser will name them)
  if (split > 0) longest = std::min(longest, split);
  c.records = fullRecords; c.bytes = fullBytes; c.sections = fullSections; c.longest = longest; c.consume = (size_t)fullBytes;
  return true;
}

// A file's leading empty lines are dropped (the reader skips them in front of a header); then its first byte is the first header's.  -> that byte ('>' or
// '@'), 0 at the end of the input, -1 for any other byte, in the reader's words.  Nothing but the empty lines is taken from the source.
int firstHeaderByte(Source& src) {
  while (true) {
    const char* base = src.buf.data() + src.pos;
    const size_t avail = src.end - src.pos;
    const char* nl = avail ? (const char*)memchr(base, '\n', avail) : nullptr;
    if (!nl && src.fill(kTextFillBytes)) continue;
    const size_t e = nl ? (size_t)(nl - base) : avail;
    if (!nl && avail == 0) return 0;
    if (xm::fastqEmptyLine(base, 0, (long long)e)) {
      src.pos += nl ? e + 1 : e;
      src.line++;
      continue;
    }
    if (base[0] == '>' || base[0] == '@') return (unsigned char)base[0];
    g_error = src.path + ": line " + std::to_string(src.line + 1) + " is neither a FASTA nor a FASTQ header";
    return -1;
  }
}

// scanBlock for FASTA text (the rules are ../csrc/xm_fasta_rules.h): whole records from src.pos on, a record ending in front of the next line whose first byte
// is '>' or at the end of the input.  maxRecords counts records, or with a split size the sections of their bases - the sum of the trimmed lengths of their
// body lines: the cutter looks at line ends and at the bytes at a line's two ends, never at a base.  The block stops in front of the record that would pass
// maxRecords, 1 GiB or 2^26 lines, but takes at least one record; a single record beyond either limit is refused with its line.
bool scanFastaBlock(Source& src, int64_t maxRecords, Cut& c, int64_t split = 0) {
  c = Cut();
  const int first = firstHeaderByte(src);  // (only a file's first block has empty lines in front, or stands at another byte than '>')
  if (first < 0) return false;
  if (first == 0) { c.atEnd = true; return true; }
  if (first != '>') { g_error = src.path + ": line " + std::to_string(src.line + 1) + " is a FASTQ header where FASTA records were announced"; return false; }
  size_t off = 0;                         // (relative to src.pos: fill() moves the buffer)
  int64_t recLines = 0, recBases = 0;     // the record in progress
  // the record in progress ends at `to`: into the block if it fits; false: the block is full in front of it
  auto close = [&](size_t to) {
    const int64_t ns = split > 0 && recBases > 0 ? (int64_t)xm::fastqSectionCount(recBases, split) : 1;  // (a record of no bases: the parser names it)
    if (c.records > 0 && ((int64_t)to > kTextBlockLimit || c.lines + recLines > xm::XM_FASTA_MAX_LINES || c.sections + ns > maxRecords)) return false;
    c.records++; c.bytes = (int64_t)to; c.lines += recLines; c.sections += ns;
    c.longest = std::max(c.longest, recBases);
    recLines = recBases = 0;
    return true;
  };
  while (true) {
    const char* base = src.buf.data() + src.pos;
    const size_t avail = src.end - src.pos;
    if (off >= avail) {
      growAhead(src, c.records, c.bytes, maxRecords);
      if (src.fill(kTextFillBytes)) continue;
      c.atEnd = true;
      break;
    }
    if (base[off] == '>' && recLines > 0) {  // the next record's header
      if (!close(off) || c.sections >= maxRecords) break;
    }
    const char* nl = (const char*)memchr(base + off, '\n', avail - off);
    if (!nl) growAhead(src, c.records, c.bytes, maxRecords);
    if (!nl && src.fill(kTextFillBytes)) continue;
    const size_t e = nl ? (size_t)(nl - base) : avail;  // (a last line without its newline)
    recLines++;
    recBases += (int64_t)xm::fastaLineBases(base, (long long)off, (long long)e);
    off = nl ? e + 1 : e;
    if ((int64_t)off > kTextBlockLimit || recLines > xm::XM_FASTA_MAX_LINES) {
      if (c.records > 0) break;  // the block is full; the record in progress is the next block's
      g_error = src.path + ": a FASTA record of more than 1 GiB or 2^26 lines at line " + std::to_string(src.line + 1);
      return false;
    }
  }
  if (c.atEnd && recLines > 0 && !close(off)) c.atEnd = false;  // (the next block takes the last record)
  if (split > 0) c.longest = std::min(c.longest, split);
  c.consume = (size_t)c.bytes;
  return true;
}

struct TextStore { std::vector<char> a, b; };

}  // namespace

struct xmio_text_reader {
  Source a, b;
  bool paired = false;
  int64_t split = 0;  // xmio_text_open_split
  bool fasta = false;  // xmio_text_open_fasta
};

extern "C" {

xmio_text_reader* xmio_text_open(const char* path1, const char* path2) {
  xmio_text_reader* r = new xmio_text_reader();
  if (!path1 || !r->a.open(path1)) { g_error = std::string("cannot open ") + (path1 ? path1 : "(null)"); delete r; return nullptr; }
  if (path2) {
    if (!r->b.open(path2)) { g_error = std::string("cannot open ") + path2; r->a.close(); delete r; return nullptr; }
    r->paired = true;
  }
  auto adopt = [](Source& src) {  // a waiting buffer that is larger than the fresh one: the source starts in it, and need not grow to a block's size again
    std::lock_guard<std::mutex> lock(g_bufferMu);
    for (size_t i = 0; i < g_buffers.size(); i++)
      if (g_buffers[i].size() > src.buf.size()) { src.buf.swap(g_buffers[i]); g_buffers.erase(g_buffers.begin() + (long)i); return; }
  };
  adopt(r->a);
  if (r->paired) adopt(r->b);
  return r;
}

xmio_text_reader* xmio_text_open_split(const char* path, int32_t split_past_size) {
  if (split_past_size < 1 || split_past_size > xm::XM_FASTQ_MAX_MATE) { g_error = "xmio_text_open_split: split_past_size must be 1 .. 30000 (a section is a mate)"; return nullptr; }
  xmio_text_reader* r = xmio_text_open(path, nullptr);
  if (r) r->split = split_past_size;
  return r;
}

xmio_text_reader* xmio_text_open_fasta(const char* path1, const char* path2, int32_t split_past_size) {
  if (split_past_size < 0 || split_past_size > xm::XM_FASTQ_MAX_MATE) { g_error = "xmio_text_open_fasta: split_past_size must be 0 .. 30000 (a section is a mate)"; return nullptr; }
  if (split_past_size > 0 && path2) { g_error = "xmio_text_open_fasta: pairs are not cut into sections (a split size is for single reads)"; return nullptr; }
  xmio_text_reader* r = xmio_text_open(path1, path2);
  if (r) { r->fasta = true; r->split = split_past_size; }
  return r;
}

int xmio_first_header_byte(const char* path) {
  Source src;
  if (!path || !src.open(path)) return fail(std::string("cannot open ") + (path ? path : "(null)"));
  const int c = firstHeaderByte(src);
  src.close();
  return c;
}

void xmio_text_close(xmio_text_reader* r) {
  if (!r) return;
  r->a.close(); r->b.close();
  giveBuffer(r->a.buf); giveBuffer(r->b.buf);
  delete r;
}

void xmio_text_block_free(xmio_text_block* b) {
  if (!b) return;
  TextStore* st = (TextStore*)b->store;
  if (st) { giveBuffer(st->a); giveBuffer(st->b); }
  delete st;
  delete b;
}

int xmio_text_next(xmio_text_reader* r, int64_t max_queries, xmio_text_block** out) {
  *out = nullptr;
  if (max_queries < 1) return fail("xmio_text_next: max_queries must be >= 1");
  Cut a, b;
  auto scan = [r](Source& src, int64_t most, Cut& c, int64_t split) { return r->fasta ? scanFastaBlock(src, most, c, split) : scanBlock(src, most, c, split); };
  if (!scan(r->a, max_queries, a, r->split)) return -1;
  if (r->paired) {
    if (!scan(r->b, a.records > 0 ? a.records : 1, b, 0)) return -1;
    if ((a.records == 0) != (b.records == 0) || (b.records < a.records && b.atEnd)) {
      std::string where;  // (FASTA text: the line the shorter file ends at)
      if (r->fasta) {
        const bool firstEnds = a.records == 0;
        where = " (" + (firstEnds ? r->a.path : r->b.path) + " ends at line " + std::to_string((firstEnds ? r->a.line + a.lines : r->b.line + b.lines)) + ")";
      }
      return fail("paired query files have different numbers of reads: " + r->a.path + ", " + r->b.path + where);
    }
    if (b.records < a.records && !scan(r->a, b.records, a, 0)) return -1;  // (the second file's block was full first)
    if (a.records != b.records) return fail("paired query files cannot be cut in step: " + r->a.path + ", " + r->b.path);
  }
  // -> where the block's text lies: in the source's buffer, which the block then owns (the source gets another one with what is left), or in a copy
  auto take = [](Source& src, const Cut& c, std::vector<char>& hold) -> const char* {
    const char* text = src.buf.data() + src.pos;
    const size_t avail = src.end - src.pos, rest = avail - c.consume;
    src.line += c.lines ? c.lines : 4 * c.records;
    if ((size_t)c.bytes < kTextBufferBytes / 2 || rest > (size_t)c.bytes / 4) {  // a small block, or one of several in the buffer
      hold.assign(text, text + c.bytes);
      src.pos += c.consume;
      return hold.data();
    }
    std::vector<char> next = takeBuffer(src.buf.size());  // (as large as the one that goes: the next block will need as much, and a buffer that grows is copied)
    memcpy(next.data(), text + c.consume, rest);
    hold.swap(src.buf);   // (a swap keeps the bytes where they are: `text` stays valid)
    src.buf.swap(next);
    src.pos = 0; src.end = rest;
    return text;
  };
  if (a.records == 0) {  // the end of the input (what is left is empty lines)
    r->a.pos += a.consume;
    if (r->paired) r->b.pos += b.consume;
    return 0;
  }
  TextStore* st = new TextStore();
  const char* text1 = take(r->a, a, st->a);
  const char* text2 = r->paired ? take(r->b, b, st->b) : nullptr;
  xmio_text_block* blk = new xmio_text_block();
  blk->store = st;
  blk->text1 = text1; blk->bytes1 = a.bytes; blk->records1 = a.records; blk->longest1 = a.longest;
  blk->text2 = text2; blk->bytes2 = r->paired ? b.bytes : 0; blk->records2 = r->paired ? b.records : 0; blk->longest2 = r->paired ? b.longest : 0;
  blk->num_queries = a.sections;
  blk->lines1 = r->fasta ? a.lines : 4 * a.records; blk->lines2 = !r->paired ? 0 : r->fasta ? b.lines : 4 * b.records;
  blk->format = r->fasta ? XMIO_TEXT_FASTA : XMIO_TEXT_FASTQ;
  *out = blk;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- writing
namespace {

// Double.toString as mapper_amd/sam.py java_double has it: the shortest decimal that reads back as the same double, plain notation with at least one
// fractional digit for 1e-3 <= |x| < 1e7, otherwise d.dddE<n>
void javaDouble(double x, std::string& out) {
  if (x != x) { out += "NaN"; return; }
  if (x == 0) { out += "0.0"; return; }  // (sam.py: x == 0 -> "0.0", also for -0.0)
  if (x > 1.7976931348623157e308) { out += "Infinity"; return; }
  if (x < -1.7976931348623157e308) { out += "-Infinity"; return; }
  char buf[64];
  auto res = std::to_chars(buf, buf + sizeof(buf), x, std::chars_format::scientific);  // shortest round trip: d[.ddd]e[+-]xx
  std::string s(buf, res.ptr);
  size_t i = 0;
  bool neg = false;
  if (s[0] == '-') { neg = true; i = 1; }
  const size_t e = s.find('e');
  std::string digits;
  for (size_t k = i; k < e; k++) if (s[k] != '.') digits += s[k];
  const int exp10 = atoi(s.c_str() + e + 1);
  const double a = x < 0 ? -x : x;
  if (neg) out += '-';
  if (a >= 1e-3 && a < 1e7) {
    if (exp10 >= 0) {
      const size_t intDigits = (size_t)exp10 + 1;
      if (digits.size() <= intDigits) { out += digits; out.append(intDigits - digits.size(), '0'); out += ".0"; }
      else { out.append(digits, 0, intDigits); out += '.'; out.append(digits, intDigits, std::string::npos); }
    } else {
      out += "0.";
      out.append((size_t)(-exp10 - 1), '0');
      out += digits;
    }
  } else {
    out += digits[0];
    out += '.';
    if (digits.size() > 1) out.append(digits, 1, std::string::npos); else out += '0';
    out += 'E';
    out += std::to_string(exp10);
  }
}

void appendInt(std::string& out, long long v) {
  char buf[24];
  auto res = std::to_chars(buf, buf + sizeof(buf), v);
  out.append(buf, res.ptr);
}

struct SeqAl { int contig, rev, nb; const int32_t* blocks; };
struct Stats { long long aligned = 0, totalLen = 0, indels = 0; };

void appendCigar(std::string& out, const SeqAl& sa, int queryLen) {  // sam.py cigar()
  const int32_t* first = sa.blocks;
  const int32_t* last = sa.blocks + 4 * (sa.nb - 1);
  if (first[0] > 0) { appendInt(out, first[0]); out += 'S'; }  // [unpinned]
  char prevOp = 0;
  long long prevN = 0;
  for (int k = 0; k < sa.nb; k++) {
    const int32_t la = sa.blocks[4 * k + 2], lb = sa.blocks[4 * k + 3];
    char op; long long n;
    if (la == lb) { op = 'M'; n = la; } else if (lb == 0) { op = 'I'; n = la; } else { op = 'D'; n = lb; }
    if (prevOp == op) prevN += n;
    else { if (prevOp) { appendInt(out, prevN); out += prevOp; } prevOp = op; prevN = n; }
  }
  if (prevOp) { appendInt(out, prevN); out += prevOp; }
  const int tail = queryLen - (last[0] + last[2]);
  if (tail > 0) { appendInt(out, tail); out += 'S'; }  // [unpinned]
}

void appendSeq(std::string& out, const uint8_t* codes, int n, bool rev) {
  const size_t at = out.size();
  out.resize(at + (size_t)n);
  char* p = &out[at];
  if (!rev) for (int i = 0; i < n; i++) p[i] = g_decode[codes[i] & 15];
  else for (int i = 0; i < n; i++) p[i] = g_decode[g_comp[codes[n - 1 - i] & 15]];
}

// query q as it came in, to the unaligned-query file's text: FASTQ when it had qualities, else FASTA [unpinned format]
void appendUnaligned(std::string& un, const xmio_batch* b, int64_t q) {
  const int nMates = b->mate_count[q];
  for (int mate = 0; mate < nMates; mate++) {
    const int64_t m = 2 * q + mate;
    const bool fq = b->has_qual && b->has_qual[m];
    un += fq ? '@' : '>';
    un.append(b->names + b->name_off[m], (size_t)(b->name_off[m + 1] - b->name_off[m]));
    un += '\n';
    appendSeq(un, b->codes + b->mate_offset[m], b->mate_length[m], false);
    un += '\n';
    if (fq) { un += "+\n"; un.append(b->quals + b->qual_off[m], (size_t)(b->qual_off[m + 1] - b->qual_off[m])); un += '\n'; }
  }
}

struct FormatJob {
  const xmio_batch* b;
  const int32_t* ints; const double* dbls; const int64_t* intOff; const int64_t* dblOff;
  const char* const* contigs; int nContigs;
  bool wantSam, wantUnaligned;
};

// the records of queries [q0, q1) appended to sam / unaligned; false = malformed streams
bool formatRange(const FormatJob& J, int64_t q0, int64_t q1, std::string& sam, std::string& un, Stats& st) {
  const xmio_batch* b = J.b;
  for (int64_t q = q0; q < q1; q++) {
    const int32_t* ii = J.ints + J.intOff[q];
    const int32_t* iiEnd = J.ints + J.intOff[q + 1];
    const double* dd = J.dbls + J.dblOff[q];
    const int nMates = b->mate_count[q];
    const bool paired = nMates > 1;
    const int ncomp = *ii++;
    bool any = false;
    for (int c = 0; c < ncomp; c++) {
      const int nal = *ii++;
      for (int a = 0; a < nal; a++) {
        any = true;
        ii++;  // innerDistance
        const int nseq = *ii++;
        const double spacingPenalty = dd[0], penalty = dd[3];
        dd += 4;
        SeqAl sas[2];
        if (nseq < 1 || nseq > 2) return false;
        for (int k = 0; k < nseq; k++) {
          sas[k].contig = ii[0]; sas[k].rev = ii[1]; sas[k].nb = ii[2]; sas[k].blocks = ii + 3;
          ii += 3 + 4 * sas[k].nb;
          dd += 2;
          if (sas[k].nb < 1 || sas[k].contig < 0 || sas[k].contig >= J.nContigs || ii > iiEnd) return false;
          for (int j = 0; j < sas[k].nb; j++) { st.totalLen += sas[k].blocks[4 * j + 2]; if (sas[k].blocks[4 * j + 2] != sas[k].blocks[4 * j + 3]) st.indels++; }
        }
        if (!J.wantSam) continue;
        for (int k = 0; k < nseq; k++) {
          const SeqAl& sa = sas[k];
          const int mate = ncomp == 1 ? k : c;  // (a pair that fell back to unpaired alignments, AlignerWorker.java:602-644: one component per mate)
          if (mate >= nMates) return false;
          const int64_t m = 2 * q + mate;
          sam.append(b->names + b->name_off[m], (size_t)(b->name_off[m + 1] - b->name_off[m]));
          sam += '\t';
          int flag;
          const SeqAl* other = nullptr;
          if (ncomp == 1) {
            if (paired) {
              if (nseq != 2) return false;
              other = &sas[1 - k];
              flag = 1 | 2 | (sa.rev ? 0x10 : 0) | (other->rev ? 0x20 : 0) | (k == 0 ? 0x40 : 0x80);
            } else {
              flag = sa.rev ? 0x10 : 0;  // 16 is [unpinned]
            }
          } else {
            flag = 1 | 8 | (sa.rev ? 0x10 : 0) | (mate == 0 ? 0x40 : 0x80);
          }
          appendInt(sam, flag); sam += '\t';
          sam += J.contigs[sa.contig]; sam += '\t';
          appendInt(sam, (long long)sa.blocks[1] + 1); sam += "\t255\t";
          const int len = b->mate_length[m];
          appendCigar(sam, sa, len); sam += '\t';
          if (other) { sam += J.contigs[other->contig]; sam += '\t'; appendInt(sam, (long long)other->blocks[1] + 1); }
          else sam += "*\t0";
          sam += '\t';
          appendInt(sam, len); sam += '\t';
          appendSeq(sam, b->codes + b->mate_offset[m], len, sa.rev != 0);
          sam += "\t*";
          if (ncomp != 1) sam += "\tcs:f:0.0";
          else if (paired) { sam += "\tcs:f:"; javaDouble(spacingPenalty, sam); }
          sam += "\tAS:f:";
          javaDouble(penalty, sam);
          sam += '\n';
        }
      }
    }
    if (any) st.aligned++;
    else if (J.wantUnaligned) appendUnaligned(un, b, q);
  }
  return true;
}

// xmio_last_write_seconds: wall time of this thread's last xmio_write_batch call in formatting (and counting) and in write()
thread_local double g_formatSeconds = 0, g_fileSeconds = 0;
double nowSeconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool writeAll(int fd, const std::string& s) {
  size_t done = 0;
  while (done < s.size()) {
    ssize_t n = write(fd, s.data() + done, s.size() - done);
    if (n < 0) return false;
    done += (size_t)n;
  }
  return true;
}

}  // namespace

extern "C" {

// SAM records (no header) of a batch's result streams to sam_fd, its unaligned queries to unaligned_fd (either may be -1), in query order.
int xmio_write_batch(const xmio_batch* b, const int32_t* ints, const double* dbls, const int64_t* int_off, const int64_t* dbl_off, int32_t num_contigs,
                     const char* const* contig_names, int32_t sam_fd, int32_t unaligned_fd, int32_t threads, xmio_stats* stats) {
  if (!b || !ints || !dbls || !int_off || !dbl_off || !stats) return fail("xmio_write_batch: null argument");
  FormatJob J{b, ints, dbls, int_off, dbl_off, contig_names, num_contigs, sam_fd >= 0, unaligned_fd >= 0};
  const int64_t nq = b->num_queries;
  if (threads < 1) threads = 1;
  const int64_t chunk = 4096;
  const int64_t nChunks = (nq + chunk - 1) / chunk;
  // chunks are formatted by the threads in any order and written in order, a window of them at a time (memory stays O(window))
  const int64_t window = std::max<int64_t>((int64_t)threads * 4, 8);
  std::vector<std::string> sam((size_t)window), un((size_t)window);
  std::vector<Stats> st((size_t)nChunks);
  std::atomic<bool> bad(false);
  const double tStart = nowSeconds();
  double fileSeconds = 0;
  g_formatSeconds = g_fileSeconds = 0;
  for (int64_t w0 = 0; w0 < nChunks; w0 += window) {
    const int64_t w1 = std::min(nChunks, w0 + window);
    std::atomic<int64_t> next(w0);
    auto work = [&]() {
      while (true) {
        const int64_t c = next.fetch_add(1);
        if (c >= w1) break;
        std::string& s = sam[(size_t)(c - w0)];
        std::string& u = un[(size_t)(c - w0)];
        s.clear(); u.clear();
        if (!formatRange(J, c * chunk, std::min(nq, (c + 1) * chunk), s, u, st[(size_t)c])) bad = true;
      }
    };
    const int nt = (int)std::min<int64_t>(threads, w1 - w0);
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (bad) return fail("xmio_write_batch: malformed result streams");
    const double tWrite = nowSeconds();
    for (int64_t c = w0; c < w1; c++) {
      if (sam_fd >= 0 && !writeAll(sam_fd, sam[(size_t)(c - w0)])) return fail("xmio_write_batch: write to the SAM file failed");
      if (unaligned_fd >= 0 && !writeAll(unaligned_fd, un[(size_t)(c - w0)])) return fail("xmio_write_batch: write to the unaligned-query file failed");
    }
    fileSeconds += nowSeconds() - tWrite;
  }
  long long aligned = 0, totalLen = 0, indels = 0;
  for (auto& s : st) { aligned += s.aligned; totalLen += s.totalLen; indels += s.indels; }
  // the penalties in query order, as Mapper.run sums them (a double sum: the order is part of the result)
  double totalPenalty = stats->total_penalty;
  for (int64_t q = 0; q < nq; q++) {
    const int32_t* ii = ints + int_off[q];
    const double* dd = dbls + dbl_off[q];
    const int ncomp = *ii++;
    for (int c = 0; c < ncomp; c++) {
      const int nal = *ii++;
      for (int a = 0; a < nal; a++) {
        const int nseq = ii[1];
        ii += 2;
        totalPenalty += dd[3];
        dd += 4;
        for (int k = 0; k < nseq; k++) { ii += 3 + 4 * ii[2]; dd += 2; }
      }
    }
  }
  stats->num_queries += nq;
  stats->num_aligned += aligned;
  stats->total_aligned_length += totalLen;
  stats->num_indels += indels;
  stats->total_penalty = totalPenalty;
  g_fileSeconds = fileSeconds;
  g_formatSeconds = nowSeconds() - tStart - fileSeconds;
  return 0;
}

// What xmio_write_batch does with sam_fd = -1, from a summary of the streams instead of the streams (xm_summary_last of include/xmapper_hip.h): the unaligned
// queries of the list to unaligned_fd, and the statistics.
int xmio_write_summary(const xmio_batch* b, int64_t num_aligned, int64_t total_aligned_length, int64_t num_indels, int64_t num_alignments, const double* penalties,
                       int64_t num_unaligned, const int64_t* unaligned, int32_t unaligned_fd, xmio_stats* stats) {
  if (!b || !stats) return fail("xmio_write_summary: null argument");
  if (num_alignments < 0 || num_unaligned < 0 || (num_alignments > 0 && !penalties) || (num_unaligned > 0 && !unaligned)) return fail("xmio_write_summary: a count without its array");
  const int64_t nq = b->num_queries;
  const double tStart = nowSeconds();
  double fileSeconds = 0;
  g_formatSeconds = g_fileSeconds = 0;
  for (int64_t i = 0; i < num_unaligned; i++)
    if (unaligned[i] < 0 || unaligned[i] >= nq || (i > 0 && unaligned[i] <= unaligned[i - 1]))
      return fail("xmio_write_summary: the list of unaligned queries is not strictly ascending inside the batch (entry " + std::to_string(i) + ")");
  if (unaligned_fd >= 0 && num_unaligned > 0 && (!b->names || !b->codes || !b->name_off || !b->mate_count || !b->mate_offset || !b->mate_length))
    return fail("xmio_write_summary: the batch has no names or codes on the host (it stayed in HBM: xm_context_set_batch_copy(0)), so its unaligned queries cannot be written from it "
                "(write the text of xm_unaligned_format_last and pass unaligned_fd = -1)");
  if (unaligned_fd >= 0) {
    std::string un;
    for (int64_t i = 0; i < num_unaligned; i++) {
      appendUnaligned(un, b, unaligned[i]);
      if (un.size() >= (size_t)(8 << 20) || i + 1 == num_unaligned) {  // (memory stays bounded)
        const double tWrite = nowSeconds();
        if (!writeAll(unaligned_fd, un)) return fail("xmio_write_summary: write to the unaligned-query file failed");
        fileSeconds += nowSeconds() - tWrite;
        un.clear();
      }
    }
  }
  // the penalties in query order, as Mapper.run sums them (a double sum: the order is part of the result)
  double totalPenalty = stats->total_penalty;
  for (int64_t a = 0; a < num_alignments; a++) totalPenalty += penalties[a];
  stats->num_queries += nq;
  stats->num_aligned += num_aligned;
  stats->total_aligned_length += total_aligned_length;
  stats->num_indels += num_indels;
  stats->total_penalty = totalPenalty;
  g_fileSeconds = fileSeconds;
  g_formatSeconds = nowSeconds() - tStart - fileSeconds;
  return 0;
}

void xmio_last_write_seconds(double* format_seconds, double* file_seconds) {
  if (format_seconds) *format_seconds = g_formatSeconds;
  if (file_seconds) *file_seconds = g_fileSeconds;
}

// Double.toString of x as the SAM tags print it (tests)
int xmio_java_double(double x, char* out, int32_t cap) {
  std::string s;
  javaDouble(x, s);
  if ((int)s.size() + 1 > cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

}  // extern "C"
