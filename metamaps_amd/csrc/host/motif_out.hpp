// mapDirectly --mods LIST --mod-motifs M1,M2,... [--mod-motif-min-frac F] [--mod-motif-combine-strands] (not in the reference): PREFIX.motifs.bedmethyl and
// PREFIX.motifs.tsv, which motifs of which contig are methylated and at what fraction of their occurrences (the definition: csrc/mm_motif_core.hpp).  Both are
// plain text whatever --compress-output says; an empty run and a query without tags write the first empty and the header of the second alone.
//   items       1 to 8 comma-separated MOTIF:OFFSET: 1 to 32 upper-case IUPAC letters and the 0-based place of the modified base, which is one of A C G T and
//               the base of at least one code of --mods.  An item's place in the list is its index; duplicates are refused.
//   F           a decimal in [0, 1], default 0.5: an occurrence is modified iff it is covered (--mod-min-coverage) and N_mod >= F * N_valid_cov.
//   combine     only with motifs that are their own reverse complement as sequences of letter sets: the two strands of a window are one unit at the + site.
//   bedmethyl   one row per covered (occurrence, code): mods_out.hpp's 18 columns with code,MOTIF,OFFSET in column 4 (a,GATC,1) and, under combined strands,
//               . as the strand; in the order contig, position, + before -, motif, code.
//   tsv         #contigID motif offset code sites covered modified N_valid_cov N_mod fraction (tab-separated): one row per (contig with an entry in the run's
//               table, motif, applicable code), then one row * per (motif, code) with those contigs' sums; fraction = "%.6f" of N_mod / N_valid_cov, NA for 0.
//   groups      mm_mod_motifs takes a range of contigs at a time: consensus_out.hpp's groups over the contigs with an entry, up to MM_MOTIF_GROUP_BASES (2^28).
// Text, arrays and the option values only: nothing here calls the device.
#pragma once
#include "../mm_motif_core.hpp"
#include "mods_out.hpp"

namespace {

struct MotifOpts {
  bool on = false, combine = false; int n = 0; double min_frac = mmt::DEFAULT_MIN_FRAC;
  std::string text[mmt::MAX_MOTIFS];                               // the letters as given
  std::vector<int32_t> off{0}, pos; std::vector<uint8_t> mask;     // as mm_mod_motifs takes them
};
// own reverse complement as a sequence of letter sets (whatever the offset)
bool motif_own_reverse_complement(const std::string& letters) {
  for (size_t i = 0; i < letters.size(); ++i)
    if (mmt::letter_mask((uint8_t)letters[i]) != mmt::comp_mask(mmt::letter_mask((uint8_t)letters[letters.size() - 1 - i]))) return false;
  return true;
}
// validated before any work; all three are refused without --mods, the two optional ones without --mod-motifs
MotifOpts motif_options(const Options& o, const ModsOpts& mo) {
  MotifOpts m;
  m.on = o.v.count("mod-motifs") != 0;
  for (const char* name : {"mod-motifs", "mod-motif-min-frac", "mod-motif-combine-strands"}) if (o.v.count(name) && !mo.on) die(std::string("--") + name + " needs --mods");
  for (const char* name : {"mod-motif-min-frac", "mod-motif-combine-strands"}) if (o.v.count(name) && !m.on) die(std::string("--") + name + " needs --mod-motifs");
  if (!m.on) return m;
  const std::string& list = o.v.at("mod-motifs");
  for (size_t a = 0; a <= list.size();) {
    const size_t e = std::min(list.find(',', a), list.size());
    const std::string it = list.substr(a, e - a);
    const size_t colon = it.find(':');
    const std::string letters = it.substr(0, colon), num = colon == std::string::npos ? "" : it.substr(colon + 1);
    if (letters.empty() || letters.size() > (size_t)mmt::MAX_LEN || letters.find_first_not_of("ACGTRYSWKMBDHVN") != std::string::npos ||
        !integer_value(num, 2).ok || m.n == mmt::MAX_MOTIFS)
      die("--mod-motifs takes 1 to 8 comma-separated items MOTIF:OFFSET (1 to 32 IUPAC letters of ACGTRYSWKMBDHVN, ':', the 0-based place of the modified base), not '" + it + "' in '" +
          list + "'");
    const int pos = (int)integer_value(num, 2).value;
    if (pos >= (int)letters.size()) die("--mod-motifs: the item " + it + ": the offset " + num + " is not inside the motif's " + std::to_string(letters.size()) + " letters");
    if (!strchr("ACGT", letters[(size_t)pos])) die("--mod-motifs: the item " + it + ": the modified base " + std::string(1, letters[(size_t)pos]) + " is not one of A C G T");
    if (std::find(mo.code_base, mo.code_base + mo.n_codes, (uint8_t)letters[(size_t)pos]) == mo.code_base + mo.n_codes)
      die("--mod-motifs: the item " + it + ": no code of --mods has the base " + std::string(1, letters[(size_t)pos]));
    for (int k = 0; k < m.n; ++k) if (m.text[k] == letters && m.pos[(size_t)k] == pos) die("--mod-motifs: the item " + it + " is given twice");
    m.text[m.n++] = letters; m.pos.push_back(pos);
    for (char c : letters) m.mask.push_back((uint8_t)mmt::letter_mask((uint8_t)c));
    m.off.push_back((int32_t)m.mask.size());
    a = e + 1;
  }
  if (o.v.count("mod-motif-min-frac")) {
    const std::string& v = o.v.at("mod-motif-min-frac");
    const DecimalValue x = decimal_value(v);
    if (!x.ok || !(x.value >= 0.0 && x.value <= 1.0)) die("--mod-motifs: --mod-motif-min-frac takes a decimal from 0 to 1, not '" + v + "'");
    m.min_frac = x.value;
  }
  if (o.v.count("mod-motif-combine-strands")) {
    for (int k = 0; k < m.n; ++k)
      if (!motif_own_reverse_complement(m.text[k])) die("--mod-motif-combine-strands: the motif " + m.text[k] + " is not its own reverse complement");
    m.combine = true;
  }
  return m;
}

// the rows of mm_mod_motifs appended as lines of PREFIX.motifs.bedmethyl
void motif_bedmethyl_text(const ModsOpts& mo, const MotifOpts& mt, const std::vector<uint64_t>& site, const std::vector<int32_t>& motif, const std::vector<int32_t>& code,
                          const std::vector<uint64_t>& n_mod, const std::vector<uint64_t>& n_canonical, const std::vector<uint64_t>& n_other, const std::vector<uint64_t>& n_fail,
                          const std::vector<std::string>& cname, std::string& t) {
  char pct[32];
  for (size_t i = 0; i < site.size(); ++i) {
    const long long pos = (long long)mmd::key_pos(site[i]);
    const unsigned long long valid = n_mod[i] + n_canonical[i] + n_other[i];
    auto num = [&](unsigned long long v) { append_int(t, (long long)v); t += '\t'; };
    t += cname[(size_t)mmd::key_contig(site[i])]; t += '\t'; num((unsigned long long)pos); num((unsigned long long)pos + 1);
    t += mo.code_name[code[i]]; t += ','; t += mt.text[motif[i]]; t += ','; append_int(t, mt.pos[(size_t)motif[i]]); t += '\t';
    num(valid); t += mt.combine ? '.' : mmd::key_minus(site[i]) ? '-' : '+'; t += '\t'; num((unsigned long long)pos); num((unsigned long long)pos + 1); t += "255,0,0\t"; num(valid);
    snprintf(pct, sizeof pct, "%.2f", valid ? 100.0 * (double)n_mod[i] / (double)valid : 0.0);
    t += pct; t += '\t'; num(n_mod[i]); num(n_canonical[i]); num(n_other[i]); t += "0\t"; num(n_fail[i]); t += "0\t0\n";
  }
}

std::string motif_tsv_header() { return "#contigID\tmotif\toffset\tcode\tsites\tcovered\tmodified\tN_valid_cov\tN_mod\tfraction\n"; }
void motif_tsv_row(const std::string& contig_id, const ModsOpts& mo, const MotifOpts& mt, int motif, int code, const int64_t* sums, std::string& t) {
  t += contig_id; t += '\t'; t += mt.text[motif]; t += '\t'; append_int(t, mt.pos[(size_t)motif]); t += '\t'; t += mo.code_name[code];
  for (int k = 0; k < mmt::SUMS; ++k) { t += '\t'; append_int(t, (long long)sums[k]); }
  char f[32];
  if (sums[3] > 0) snprintf(f, sizeof f, "%.6f", (double)sums[4] / (double)sums[3]); else snprintf(f, sizeof f, "NA");
  t += '\t'; t += f; t += '\n';
}
// The summary of one mm_mod_motifs call appended as lines of PREFIX.motifs.tsv, and added to the sums of the * rows: total[(motif * MAX_CODES + code) * SUMS ...].
void motif_tsv_text(const ModsOpts& mo, const MotifOpts& mt, const std::vector<int32_t>& contig, const std::vector<int32_t>& motif, const std::vector<int32_t>& code,
                    const std::vector<int64_t>& sums, const std::vector<std::string>& cname, std::vector<int64_t>& total, std::string& t) {
  total.resize((size_t)mmt::MAX_MOTIFS * mmd::MAX_CODES * mmt::SUMS, 0);
  for (size_t i = 0; i < contig.size(); ++i) {
    motif_tsv_row(cname[(size_t)contig[i]], mo, mt, motif[i], code[i], &sums[i * mmt::SUMS], t);
    for (int k = 0; k < mmt::SUMS; ++k) total[((size_t)motif[i] * mmd::MAX_CODES + (size_t)code[i]) * mmt::SUMS + (size_t)k] += sums[i * mmt::SUMS + (size_t)k];
  }
}
// the rows * behind the contigs' (none where no contig was listed: an empty run writes the header alone)
void motif_tsv_totals(const ModsOpts& mo, const MotifOpts& mt, const std::vector<int64_t>& total, std::string& t) {
  if (total.empty()) return;
  for (int j = 0; j < mt.n; ++j)
    for (int c = 0; c < mo.n_codes; ++c)
      if (mo.code_base[c] == (uint8_t)mt.text[j][(size_t)mt.pos[(size_t)j]]) motif_tsv_row("*", mo, mt, j, c, &total[((size_t)j * mmd::MAX_CODES + (size_t)c) * mmt::SUMS], t);
}

}  // namespace
