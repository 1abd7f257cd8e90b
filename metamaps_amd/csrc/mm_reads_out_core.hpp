// FASTQ / FASTA records of selected reads of a sequence set (mapDirectly --extract-* / --deplete-taxa; mm_reads_encode; DESIGN.md section 1, "Read
// extraction"): the size of one record, the byte at every offset of it and the three rules, written once for the kernels of mm_reads_out.hip (one
// wavefront per record) and for the host (plain g++: tests/test_reads_out_core.cpp holds it to tests/reads_out_ref.py byte for byte).
//
//   record   with_qual:  '@' name '\n' bases '\n' '+' '\n' qual '\n'      (2 m + l_name + 6 bytes for a read of m bases)
//            without:    '>' name '\n' bases '\n'                          (m + l_name + 3 bytes); the bases are never wrapped
//   bases    the bytes the set holds, in the read's own orientation: upper-cased at upload, a byte other than A C G T verbatim from its exception run,
//            an nt16 code as its letter (a record added with reverse != 0 was turned back by the set).  Nothing is reverse-complemented here.
//   qual     the plane's Phred value + 33; a base without quality (plane byte 0xFF, or a set without a plane) is '!'.  A declared choice: a FASTQ record
//            must have as many quality characters as bases, and '!' (Phred 0) is the value that claims nothing.
//   rules    numbered as READS_RULE_*; the call is refused for the lowest record that breaks one, and for that record the lowest rule.
//
// Q gives q.byte(i), the read's byte i as stored, and q.qual(i), the stored quality of base i (0xFF: none); the host's source is QualBytes.
// Bounds: record_byte reads name[0, l_name), q.byte(0 .. m - 1) and q.qual(0 .. m - 1) and nothing else; off lies in [0, record_size).  check reads
// name[0, l_name) only when 1 <= l_name <= 254.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mmr {

constexpr int64_t NAME_BYTES_MAX = 254;
constexpr uint8_t QUAL_NONE = 0xFF;

enum Rule : int {                                                 // mm_reads_encode's refusals
  READS_OK = 0,
  READS_RULE_SET = 1,                                             // a read outside the set
  READS_RULE_NAME = 2,                                            // a name of 0 or more than 254 bytes
  READS_RULE_BYTE = 3,                                            // a name byte outside 0x21..0x7E
};
MM_HD const char* rule_text(int rule) {
  switch (rule) {
    case READS_RULE_SET: return "rule 1: the read lies outside the set";
    case READS_RULE_NAME: return "rule 2: the name has 0 or more than 254 bytes";
    case READS_RULE_BYTE: return "rule 3: a byte of the name lies outside 0x21..0x7E";
    default: return "no rule";
  }
}

MM_HD int check(int64_t read, int64_t n_reads, const char* name, int64_t l_name) {
  if (read < 0 || read >= n_reads) return READS_RULE_SET;
  if (l_name < 1 || l_name > NAME_BYTES_MAX) return READS_RULE_NAME;
  for (int64_t i = 0; i < l_name; ++i) { const uint8_t b = (uint8_t)name[i]; if (b < 0x21 || b > 0x7E) return READS_RULE_BYTE; }
  return READS_OK;
}

MM_HD int64_t record_size(int64_t l_name, int64_t m, bool with_qual) { return with_qual ? 2 * m + l_name + 6 : m + l_name + 3; }
MM_HD int64_t bases_at(int64_t l_name) { return l_name + 2; }                       // the offset of the first base
MM_HD int64_t qual_at(int64_t l_name, int64_t m) { return l_name + m + 5; }         // with_qual: the offset of the first quality character
MM_HD uint8_t qual_char(uint8_t q) { return q == QUAL_NONE ? (uint8_t)'!' : (uint8_t)(q + 33); }

// the byte at offset off of the record
template <class Q> MM_HD uint8_t record_byte(const Q& q, const char* name, int64_t l_name, int64_t m, bool with_qual, int64_t off) {
  if (off == 0) return with_qual ? (uint8_t)'@' : (uint8_t)'>';
  if (off <= l_name) return (uint8_t)name[off - 1];
  const int64_t b = off - bases_at(l_name);
  if (b < 0) return (uint8_t)'\n';
  if (b < m) return q.byte(b);
  if (b == m) return (uint8_t)'\n';
  if (b == m + 1) return (uint8_t)'+';                            // (with_qual alone gets here: the FASTA record ends at b == m)
  if (b == m + 2) return (uint8_t)'\n';
  const int64_t k = off - qual_at(l_name, m);
  return k < m ? qual_char(q.qual(k)) : (uint8_t)'\n';
}

// the record at dst, by lanes (the policies of mm_bam_core.hpp); returns its size
template <class P, class Q> MM_HD int64_t write_record(P& p, const Q& q, const char* name, int64_t l_name, int64_t m, bool with_qual, uint8_t* dst) {
  const int64_t size = record_size(l_name, m, with_qual);
  for (int64_t i = p.lane(); i < size; i += P::W) dst[i] = record_byte(q, name, l_name, m, with_qual, i);
  return size;
}

struct QualBytes {                                                // the host's source: the read's bytes and its stored qualities (null: none)
  const uint8_t* b; const uint8_t* q;
  uint8_t byte(int64_t i) const { return b[i]; }
  uint8_t qual(int64_t i) const { return q ? q[i] : QUAL_NONE; }
};
struct HostLanes {                                                // the host's lane policy: one lane
  static constexpr uint32_t W = 1;
  uint32_t lane() const { return 0; }
};

}  // namespace mmr
