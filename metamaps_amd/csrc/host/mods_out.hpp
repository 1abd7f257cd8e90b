// mapDirectly --mods LIST [--mod-min-ml T] [--mod-min-coverage N] (implies --edit-distance; not in the reference): PREFIX.bedmethyl, for every reference
// position and strand how many primary alignments carry a confident modified, canonical, other-modification or failed call there (the definition:
// csrc/mm_mods_core.hpp; the tags: SAM tags specification, "Base modifications").  The file is plain text whatever --compress-output says.
//   LIST        1 to 4 comma-separated items B+code, B one of A C G T and code lower-case letters or a ChEBI number (C+m,C+h,A+a,C+21839): the head of an MM
//               group.  An item's place in the list is its code's index; duplicates are refused.
//   tags        MM:Z is groups  B(+|-)codes[.?]?(,skip)*;  and ML:B:C one byte per (skip, code) in MM's order.  A group of several codes (C+mh) becomes one
//               group per code with the same skips, its ML bytes de-interleaved.  A group of strand - or of base N is dropped, and so is a read whose MN
//               differs from its length; U is read as T; a code that is not in LIST keeps its group with index -1.  Malformed (an error that names the
//               file and the read): a bad group syntax, an ML length other than the groups' skips add up to, a tag of another type, the same base, strand
//               and code in two groups, more than 255 groups.
//   bedmethyl   modkit's 18 tab-separated columns without a header:
//               contigID pos pos+1 code N_valid_cov strand pos pos+1 255,0,0 N_valid_cov pct N_mod N_canonical N_other_mod 0 N_fail 0 0
//               with pct = "%.2f" of 100 N_mod / N_valid_cov; columns 15, 17 and 18 (N_delete, N_diff, N_nocall) are written 0.
// Text, arrays and the option values only: nothing here calls the device.
#pragma once
#include "../mm_mods_core.hpp"
#include "bam_reader.hpp"
#include "cli_common.hpp"
#include "fast_format.hpp"
#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace {

struct ModsOpts {
  bool on = false; int n_codes = 0; std::string code_name[mmd::MAX_CODES]; uint8_t code_base[mmd::MAX_CODES] = {0, 0, 0, 0};
  int min_ml = mmd::DEFAULT_MIN_ML; long long min_coverage = 1;
};
// validated before any work; the two thresholds are refused without --mods
ModsOpts mods_options(const Options& o) {
  ModsOpts m;
  m.on = o.v.count("mods") != 0;
  if (m.on) {
    const std::string& list = o.v.at("mods");
    for (size_t a = 0; a <= list.size();) {
      const size_t e = std::min(list.find(',', a), list.size());
      const std::string it = list.substr(a, e - a);
      const std::string code = it.size() > 2 ? it.substr(2) : "";
      const bool letters = !code.empty() && code.find_first_not_of("abcdefghijklmnopqrstuvwxyz") == std::string::npos;
      if (it.size() < 3 || !strchr("ACGT", it[0]) || it[1] != '+' || !(letters || integer_value(code, 9).ok) || m.n_codes == mmd::MAX_CODES)
        die("--mods takes 1 to 4 comma-separated items like C+m, C+h, A+a or C+21839 (a base of A C G T, '+', lower-case letters or a ChEBI number), not '" + list + "'");
      for (int k = 0; k < m.n_codes; ++k) if (m.code_base[k] == (uint8_t)it[0] && m.code_name[k] == code) die("--mods: the item " + it + " is given twice");
      m.code_base[m.n_codes] = (uint8_t)it[0]; m.code_name[m.n_codes++] = code;
      a = e + 1;
    }
  }
  if (o.v.count("mod-min-ml")) {
    const std::string& v = o.v.at("mod-min-ml");
    if (!m.on) die("--mod-min-ml needs --mods");
    const IntegerValue x = integer_value(v, 3);
    if (!x.ok || x.value > 255) die("--mods: --mod-min-ml takes an integer from 0 to 255, not '" + v + "'");
    m.min_ml = (int)x.value;
  }
  if (o.v.count("mod-min-coverage")) {
    const std::string& v = o.v.at("mod-min-coverage");
    if (!m.on) die("--mod-min-coverage needs --mods");
    const IntegerValue x = integer_value(v, 9);
    if (!x.ok || x.value < 1) die("--mods: --mod-min-coverage takes an integer from 1 to 999999999, not '" + v + "'");
    m.min_coverage = (long long)x.value;
  }
  return m;
}

// a read's groups as mm_seqset_add_mods takes them (off starts at 0)
struct ModGroups {
  std::vector<uint8_t> base, mode, ml; std::vector<int8_t> code; std::vector<int64_t> off{0}; std::vector<uint32_t> skips;
  void clear() { base.clear(); mode.clear(); ml.clear(); code.clear(); off.assign(1, 0); skips.clear(); }
};
struct ModCounters { size_t reads = 0, with_tags = 0, minus_groups = 0, n_groups = 0, mn_mismatch = 0; };   // per query file, for its INFO line
struct ModTagError : std::runtime_error { using std::runtime_error::runtime_error; };

// The groups of a record's MM / ML / MN fields (type 0: absent) into g; false: the read carries no groups (no MM tag, or an MN that differs from
// l_seq).  Throws ModTagError with what is malformed.
bool mods_parse(const ModsOpts& mo, const bam::AuxField& mm, const bam::AuxField& ml, const bam::AuxField& mn, int64_t l_seq, ModGroups& g, ModCounters& n) {
  g.clear();
  if (mm.type && mm.type != 'Z') throw ModTagError("the MM tag has type " + std::string(1, mm.type) + ", not Z");
  if (ml.type && (ml.type != 'B' || ml.sub != 'C')) throw ModTagError("the ML tag is not an array of type B:C");
  if (mn.type && !strchr("cCsSiI", mn.type)) throw ModTagError("the MN tag has type " + std::string(1, mn.type) + ", not an integer");
  if (!mm.type) { if (ml.type) throw ModTagError("an ML tag without an MM tag"); return false; }
  const char* p = (const char*)mm.p; const char* const end = p + mm.bytes;
  const uint8_t* mlp = ml.p; size_t ml_left = ml.type ? ml.count : 0;
  std::vector<std::string> seen;                                   // base, strand and code of the groups so far
  std::vector<uint32_t> skips;
  const std::string text(p, mm.bytes);
  auto bad = [&](const char* what) { return ModTagError(std::string("malformed MM tag (") + what + "): " + text); };
  while (p < end) {
    char base = *p++;
    if (!strchr("ACGTUN", base)) throw bad("a group does not start with one of A C G T U N");
    if (base == 'U') base = 'T';
    if (p >= end || (*p != '+' && *p != '-')) throw bad("no strand behind the base");
    const char strand = *p++;
    const char* c0 = p;
    if (p < end && *p >= '0' && *p <= '9') while (p < end && *p >= '0' && *p <= '9') ++p;
    else while (p < end && *p >= 'a' && *p <= 'z') ++p;
    if (p == c0) throw bad("no code behind the strand");
    std::vector<std::string> codes;
    if (*c0 >= '0' && *c0 <= '9') codes.emplace_back(c0, p); else for (const char* c = c0; c < p; ++c) codes.emplace_back(1, *c);
    uint8_t mode = mmd::MODE_ABSENT;
    if (p < end && (*p == '.' || *p == '?')) mode = (uint8_t)*p++;
    skips.clear();
    while (p < end && *p == ',') {
      ++p;
      uint64_t v = 0; const char* d0 = p;
      while (p < end && *p >= '0' && *p <= '9' && v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(*p++ - '0');
      if (p == d0 || v > 0xFFFFFFFFull) throw bad("a skip is not a number below 2^32");
      skips.push_back((uint32_t)v);
    }
    if (p >= end || *p != ';') throw bad("a group does not end with ';'");
    ++p;
    const size_t nc = codes.size(), need = skips.size() * nc;
    if (need > ml_left) throw ModTagError("the ML tag holds " + std::to_string(ml.type ? ml.count : 0) + " bytes, fewer than the MM groups' skips add up to");
    for (size_t c = 0; c < nc; ++c) {
      const std::string id = std::string(1, base) + strand + codes[c];
      if (std::find(seen.begin(), seen.end(), id) != seen.end()) throw ModTagError("the code " + id + " is in two groups of the MM tag");
      seen.push_back(id);
      if (strand == '-') { ++n.minus_groups; continue; }
      if (base == 'N') { ++n.n_groups; continue; }
      if (g.base.size() == (size_t)mmd::MAX_GROUPS) throw ModTagError("more than 255 groups in one MM tag");
      int k = -1;
      for (int q = 0; q < mo.n_codes; ++q) if (mo.code_base[q] == (uint8_t)base && mo.code_name[q] == codes[c]) k = q;
      g.base.push_back((uint8_t)base); g.code.push_back((int8_t)k); g.mode.push_back(mode);
      g.skips.insert(g.skips.end(), skips.begin(), skips.end());
      for (size_t j = 0; j < skips.size(); ++j) g.ml.push_back(mlp[j * nc + c]);
      g.off.push_back((int64_t)g.skips.size());
    }
    mlp += need; ml_left -= need;
  }
  if (ml_left) throw ModTagError("the ML tag holds " + std::to_string(ml.count) + " bytes, more than the MM groups' skips add up to");
  if (mn.type && bam::aux_int(mn) != l_seq) { ++n.mn_mismatch; g.clear(); return false; }
  return true;
}

// the kept rows of mm_mod_finish as PREFIX.bedmethyl
std::string bedmethyl_text(const ModsOpts& mo, const std::vector<uint64_t>& site, const std::vector<uint64_t>& n_mod, const std::vector<uint64_t>& n_canonical,
                           const std::vector<uint64_t>& n_other, const std::vector<uint64_t>& n_fail, const std::vector<std::string>& cname) {
  std::string t;
  t.reserve(site.size() * 80);
  char pct[32];
  for (size_t i = 0; i < site.size(); ++i) {
    const long long pos = (long long)mmd::key_pos(site[i]);
    const unsigned long long valid = n_mod[i] + n_canonical[i] + n_other[i];
    auto num = [&](unsigned long long v) { append_int(t, (long long)v); t += '\t'; };
    t += cname[(size_t)mmd::key_contig(site[i])]; t += '\t'; num((unsigned long long)pos); num((unsigned long long)pos + 1); t += mo.code_name[mmd::key_class(site[i])]; t += '\t';
    num(valid); t += mmd::key_minus(site[i]) ? '-' : '+'; t += '\t'; num((unsigned long long)pos); num((unsigned long long)pos + 1); t += "255,0,0\t"; num(valid);
    snprintf(pct, sizeof pct, "%.2f", valid ? 100.0 * (double)n_mod[i] / (double)valid : 0.0);
    t += pct; t += '\t'; num(n_mod[i]); num(n_canonical[i]); num(n_other[i]); t += "0\t"; num(n_fail[i]); t += "0\t0\n";
  }
  return t;
}

}  // namespace
