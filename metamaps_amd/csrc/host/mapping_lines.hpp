// The mapping lines of one `classify` run before any table or device is involved: a line as classify sees it (MapLine), the form in which mapDirectly
// --then-classify hands its lines over in memory (LineMeta, KeptLines), the two ways to the lines of a run (tokenise a file's text in pieces; adopt the
// kept lines) and the cut of the reads into EM shards.  The standard library only (no C ABI, no device context): tests/test_mapping_lines.cpp compiles this
// and classify_tables.hpp on their own.
#pragma once
#include "cli_common.hpp"
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <new>
#include <string_view>
#include <unordered_map>

namespace {

// A mapping line as `classify` sees it once it has tokenised the file (fEM.h:234-275): where the line lies in the text, and the values of the fields it reads
// — identity and mapping quality as the PRINTED text parses, not as the floats they were printed from.  `mapDirectly --then-classify` keeps these beside the
// text it writes, so that classify in the same process neither reads the file back nor tokenises it.
struct LineMeta {
  uint32_t beg, ls /* the blank before field 14, relative to beg */, n /* length without the newline */;
  int32_t contig /* index into the reference's contigs */, len, start, stop /* field 9: start + len - 1, or its raw translation with --hpc */;
  double ident, mapq;
};
struct KeptLines {                                               // the mapping lines of one output prefix as mapDirectly wrote them, batch after batch, with their parsed fields
  struct Part { const char* text; const LineMeta* meta; size_t n_lines; const int64_t* off; size_t n_reads; };
  std::vector<Part> parts; const std::vector<std::string>* cname = nullptr;
};
struct MapLine { const char* p; uint32_t last_space, n; int contig; long long len; size_t start, stop; double ident, mapq; };   // [p, p + n): the line; p + last_space: the blank before field 14
inline std::string_view read_id(const MapLine& L) { return std::string_view(L.p, (size_t)((const char*)memchr(L.p, ' ', L.n) - L.p)); }   // field 1

struct TextBuf {                                                 // a file's bytes + a terminating 0, not zero-filled first (std::string::resize spent 0.1 s on that per 0.5 GB)
  char* p = nullptr; size_t n = 0;
  void resize(size_t k) { p = new (std::nothrow) char[k + 1]; if (!p) die("out of host memory for the mappings file"); n = k; p[k] = 0; }   // (huge_new.hpp: on huge pages)
  size_t size() const { return n; } const char* c_str() const { return p; } char& operator[](size_t i) { return p[i]; }
  ~TextBuf() { delete[] p; }
};

// What tokenise() or adopt() make of a run's input, and all that the later stages know of it
struct MappingLines {
  std::vector<MapLine> lines; std::vector<int64_t> off{0};       // read r owns lines [off[r], off[r+1])
  std::vector<std::string> contig_id; std::unordered_map<std::string, int> contig_index;   // interned in the order of their first line
  size_t NRD = 0;                                                // reads with a line
};

// In how many pieces the tokeniser cuts the text and the formatter the lines (MM_CLASSIFY_THREADS=n, `forced`: exactly n, whatever the size — the tests cut
// small inputs into many), else one per `unit` of the input within the width of the pools that compute flat out
inline size_t piece_count(size_t forced, size_t wide, size_t n, size_t unit) { return forced ? forced : std::max<size_t>(1, std::min<size_t>({(size_t)32, wide, n / unit + 1})); }

// Field 14 as the tokeniser reads it: strtod where the text lies (it ends at a blank, a newline or the buffer's 0).  taxonomy.hpp's
// mapq_as_classify_reads_it, which mapDirectly --then-classify applies to the text it has just printed, returns the same double wherever both return one
// (parse_g6_text is strtod for the shapes it takes, the rest is strtod itself, and both take 0 for an "…e-…" that strtod reports out of range: std::stod
// throws there, also on a denormal, and the reference then takes 0, fEM.h:269-275).  They differ where this one ends the program and that one cannot be
// reached, since mapDirectly prints no such text: a field that is not a number (that one: 0) and an out-of-range value without "e-" (that one: strtod's).
inline double mapq_field(const char* b, size_t n, const std::string& mapped) {
  errno = 0; char* endp = nullptr;
  double v = strtod(b, &endp);
  if (errno == ERANGE) { if (std::string(b, n).find("e-") != std::string::npos) v = 0; else die("mapping quality out of range in " + mapped); }
  if (endp == b) die("File " + mapped + " has a mapping quality that is not a number");
  return v;
}

// The text of a mappings file once through: every line is tokenised where it lies (the reference splits every line again in every EM round,
// fEM.h:1171-1214, :234-373), lines of one read are consecutive (mapWrap.h:128-149), contig IDs are interned.  `NTH` pieces of the text that begin on a
// read boundary are parsed on threads of their own and joined in file order (read offsets shifted, contig IDs interned in the order a single pass would
// meet them): 4.2 M lines took 1.3 s on one thread.  T0[TS] is 0; `mapped` names the file in the refusals.
inline MappingLines tokenise(const char* const T0, const size_t TS, const size_t NTH, const std::string& mapped) {
  // the read ID of the line that starts at p (text up to the first blank or the line's end)
  auto id_of = [&](size_t p, size_t& len) { const char* nl = (const char*)memchr(T0 + p, '\n', TS - p); const size_t e = nl ? (size_t)(nl - T0) : TS;
                                            const char* sp = (const char*)memchr(T0 + p, ' ', e - p); len = (sp ? (size_t)(sp - T0) : e) - p; };
  auto next_line = [&](size_t p) { const char* nl = (const char*)memchr(T0 + p, '\n', TS - p); return nl ? (size_t)(nl - T0) + 1 : TS; };
  // first read boundary at or after x: a line start whose ID differs from the ID of the last non-empty line before it
  auto read_boundary = [&](size_t x) {
    if (x == 0) return (size_t)0;
    size_t p = next_line(x - 1);                                  // start of the first line that begins at or after x
    while (p < TS) {
      if (T0[p] == '\n') { ++p; continue; }                       // empty line
      size_t q = p;                                              // start of the previous non-empty line
      for (;;) { if (q == 0) return p; size_t e = q - 1; size_t b0 = e; while (b0 > 0 && T0[b0 - 1] != '\n') --b0; if (e > b0) { q = b0; break; } q = b0; }
      size_t la, lb; id_of(p, la); id_of(q, lb);
      if (la != lb || memcmp(T0 + p, T0 + q, la) != 0) return p;
      p = next_line(p);
    }
    return TS;
  };
  std::vector<size_t> cut(NTH + 1, TS);
  cut[0] = 0;
  for (size_t t = 1; t < NTH; ++t) cut[t] = std::max(cut[t - 1], read_boundary(TS / NTH * t));
  struct Piece { std::vector<MapLine> lines; std::vector<int64_t> starts; std::vector<std::string> cid; std::unordered_map<std::string, int> cix; };
  std::vector<Piece> pieces(NTH);
  on_each_caller_first(NTH, [&](size_t t) {
    Piece& P = pieces[t];
    size_t cur_beg = 0, cur_len = (size_t)-1;                    // the current read's ID, as a span of the text
    for (size_t p = cut[t]; p < cut[t + 1];) {
      const char* nl = (const char*)memchr(T0 + p, '\n', cut[t + 1] - p);
      const size_t e = nl ? (size_t)(nl - T0) : cut[t + 1];
      if (e == p) { p = e + 1; continue; }                       // empty line
      size_t fb[16], fe[16]; int nf = 0;                         // fields (single blanks, util.h:80)
      for (size_t q = p; nf < 16;) { const char* sp = (const char*)memchr(T0 + q, ' ', e - q); fb[nf] = q; fe[nf] = sp ? (size_t)(sp - T0) : e; ++nf; if (!sp) break; q = fe[nf - 1] + 1; }
      if (nf < 6) die("File " + mapped + " has weird format - is this a mappings file generated by MetaMap?");
      if (nf < 14) die("File " + mapped + " has lines with fewer than 14 fields - is this a mappings file generated by MetaMap?");
      if (fe[0] - fb[0] != cur_len || memcmp(T0 + fb[0], T0 + cur_beg, cur_len) != 0) { P.starts.push_back((int64_t)P.lines.size()); cur_beg = fb[0]; cur_len = fe[0] - fb[0]; }
      MapLine L{};
      L.p = T0 + p; L.n = (uint32_t)(e - p); L.last_space = (uint32_t)(fb[13] - 1 - p);
      std::string cid(T0 + fb[5], fe[5] - fb[5]);
      auto it = P.cix.find(cid);
      if (it == P.cix.end()) { it = P.cix.emplace(cid, (int)P.cid.size()).first; P.cid.push_back(cid); }
      L.contig = it->second;
      L.len = strtoll(T0 + fb[1], nullptr, 10);
      L.start = strtoull(T0 + fb[7], nullptr, 10); L.stop = strtoull(T0 + fb[8], nullptr, 10);
      L.ident = strtod(T0 + fb[9], nullptr) / 100.0;
      L.mapq = mapq_field(T0 + fb[13], fe[13] - fb[13], mapped);
      P.lines.push_back(L);
      p = e + 1;
    }
  });
  // join: contig IDs in the order of their first line, read offsets shifted by the lines before the piece
  MappingLines M;
  std::vector<std::vector<int>> remap(NTH);
  std::vector<size_t> line0(NTH + 1, 0);
  for (size_t t = 0; t < NTH; ++t) {
    line0[t + 1] = line0[t] + pieces[t].lines.size();
    remap[t].resize(pieces[t].cid.size());
    for (size_t c = 0; c < pieces[t].cid.size(); ++c) {
      auto it = M.contig_index.find(pieces[t].cid[c]);
      if (it == M.contig_index.end()) { it = M.contig_index.emplace(pieces[t].cid[c], (int)M.contig_id.size()).first; M.contig_id.push_back(pieces[t].cid[c]); }
      remap[t][c] = it->second;
    }
  }
  M.lines.resize(line0[NTH]);
  M.off.clear();
  for (size_t t = 0; t < NTH; ++t) for (int64_t st0 : pieces[t].starts) M.off.push_back(st0 + (int64_t)line0[t]);
  if (M.off.empty()) M.off.push_back(0);
  on_each_caller_first(NTH, [&](size_t t) {
    MapLine* o = M.lines.data() + line0[t]; const auto& src = pieces[t].lines;
    for (size_t i = 0; i < src.size(); ++i) { o[i] = src[i]; o[i].contig = remap[t][(size_t)src[i].contig]; }
  });
  if (!M.lines.empty()) M.off.push_back((int64_t)M.lines.size());
  M.NRD = M.off.size() - 1;
  return M;
}

// mapDirectly --then-classify: the lines are in memory with their fields parsed (LineMeta) — what tokenise() makes of the file, without the file: read
// boundaries from the batches' offsets (reads without mappings have no lines), contig IDs interned in the order of their first line
inline MappingLines adopt(const KeptLines& kept) {
  MappingLines M;
  size_t total = 0; for (const auto& P : kept.parts) total += P.n_lines;
  M.lines.resize(total);
  M.off.clear();
  std::vector<int> intern(kept.cname->size(), -1);
  size_t at = 0;
  for (const auto& P : kept.parts) {
    for (size_t r = 0; r < P.n_reads; ++r) if (P.off[r + 1] > P.off[r]) M.off.push_back((int64_t)at + P.off[r]);
    for (size_t i = 0; i < P.n_lines; ++i) {
      const LineMeta& m = P.meta[i];
      int& ci = intern[(size_t)m.contig];
      if (ci < 0) { ci = (int)M.contig_id.size(); M.contig_id.push_back((*kept.cname)[(size_t)m.contig]); M.contig_index.emplace(M.contig_id.back(), ci); }
      M.lines[at + i] = MapLine{P.text + m.beg, m.ls, m.n, ci, (long long)m.len, (size_t)m.start, (size_t)m.stop, m.ident, m.mapq};
    }
    at += P.n_lines;
  }
  if (M.off.empty()) M.off.push_back(0);
  if (!M.lines.empty()) M.off.push_back((int64_t)M.lines.size());
  M.NRD = M.off.size() - 1;
  return M;
}

// The reads of an EM problem cut contiguously over G ranks — rank order = read order, as the reference shards them over OpenMP threads (fEM.h:1229)
struct EmShard { size_t lo = 0, hi = 0, e0 = 0; std::vector<int64_t> soff; };   // reads [lo, hi); e0: first mapping of the shard; soff: shard-local offsets
inline EmShard em_shard(const std::vector<int64_t>& off, size_t G, size_t d) {
  const size_t NR = off.size() - 1, base = NR / G, rem = NR % G;
  EmShard s;
  s.lo = d * base + std::min(d, rem); s.hi = s.lo + base + (d < rem ? 1 : 0);
  s.e0 = (size_t)off[s.lo];
  s.soff.resize(s.hi - s.lo + 1);
  for (size_t i = 0; i <= s.hi - s.lo; ++i) s.soff[i] = off[s.lo + i] - off[s.lo];
  return s;
}

}  // namespace
