"""Methylation per sequence motif (mapDirectly --mod-motifs; DESIGN.md section 1, "Modification motifs"), restated plainly: loops over contigs, positions,
strands, motifs and letters, sharing no code with metamaps_amd/csrc/mm_motif_core.hpp.  The table is mods_ref.py's {key: count}; the counts of a site
are formed as mods_ref.rows forms them."""
import mods_ref

LETTERS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
TSV_HEADER = "#contigID\tmotif\toffset\tcode\tsites\tcovered\tmodified\tN_valid_cov\tN_mod\tfraction\n"


def fits(byte, letter):
    """a reference byte (an int, as the packed set holds it: upper case) against a motif letter; a byte outside ACGT fits nothing"""
    b = chr(byte)
    return b in "ACGT" and b in LETTERS[letter]


def occurs(seq, q, strand, motif, off):
    L, n = len(motif), len(seq)
    if strand > 0:
        s = q - off
        return s >= 0 and s + L <= n and all(fits(seq[s + i], motif[i]) for i in range(L))
    s = q - (L - 1 - off)
    if s < 0 or s + L > n:
        return False
    for i in range(L):
        b = chr(seq[s + L - 1 - i])
        if b not in COMP or COMP[b] not in LETTERS[motif[i]]:
            return False
    return True


def own_reverse_complement(motif):
    return all(set(LETTERS[motif[i]]) == {COMP[x] for x in LETTERS[motif[len(motif) - 1 - i]]} for i in range(len(motif)))


def site_counts(sites, c, q, strand, k, n_codes):
    """(N_mod, N_canonical, N_other, N_fail) of code k at a site; zeros where the table has no entry"""
    cnt = sites.get((c, q, strand), {})
    return (cnt.get(3 + k, 0), cnt.get(0, 0), cnt.get(2, 0) + sum(cnt.get(3 + o, 0) for o in range(n_codes) if o != k), cnt.get(1, 0))


def profile(contigs, table, code_base, motifs, min_coverage=1, min_frac=0.5, combine=False):
    """contigs: [bytes] (upper case); table: {key: count}; motifs: [(letters, offset)].  Returns (rows, summary): rows [(contig, pos, strand, motif, code,
    n_mod, n_canonical, n_other, n_fail)] with strand 0 under combine, in the order contig, pos, + before -, motif, code; summary [(contig, motif, code, sites,
    covered, modified, n_valid_cov, n_mod)] for the contigs with an entry, in the order contig, motif, code"""
    sites = {}
    for key, n in table.items():
        c, pos, strand, cls = mods_ref.unkey(key)
        sites.setdefault((c, pos, strand), {})[cls] = n
    listed = sorted({c for c, _, _ in sites})
    rows, summary = [], []
    for c in listed:
        seq = contigs[c]
        acc = {(j, k): [0, 0, 0, 0, 0] for j, (m, o) in enumerate(motifs) for k, b in enumerate(code_base) if b == m[o]}
        for q in range(len(seq)):
            for strand in ((1,) if combine else (1, -1)):
                for j, (m, o) in enumerate(motifs):
                    if not occurs(seq, q, strand, m, o):
                        continue
                    for k, b in enumerate(code_base):
                        if b != m[o]:
                            continue
                        cnt = site_counts(sites, c, q, strand, k, len(code_base))
                        if combine:
                            assert own_reverse_complement(m)
                            q2 = (q - o) + len(m) - 1 - o
                            assert occurs(seq, q2, -1, m, o)
                            cnt = tuple(a + b for a, b in zip(cnt, site_counts(sites, c, q2, -1, k, len(code_base))))
                        a = acc[(j, k)]
                        a[0] += 1
                        valid = cnt[0] + cnt[1] + cnt[2]
                        if valid >= min_coverage:
                            a[1] += 1
                            a[2] += 1 if float(cnt[0]) >= min_frac * float(valid) else 0
                            a[3] += valid
                            a[4] += cnt[0]
                            rows.append((c, q, 0 if combine else strand, j, k) + cnt)
        summary += [(c, j, k) + tuple(acc[(j, k)]) for (j, k) in sorted(acc)]
    return rows, summary


def bedmethyl_text(rows, cname, code_name, motifs):
    """PREFIX.motifs.bedmethyl"""
    out = []
    for c, pos, strand, j, k, n_mod, n_canon, n_other, n_fail in rows:
        valid = n_mod + n_canon + n_other
        pct = "%.2f" % (100.0 * n_mod / valid) if valid else "0.00"
        name = "%s,%s,%d" % (code_name[k], motifs[j][0], motifs[j][1])
        out.append("\t".join(str(x) for x in (cname[c], pos, pos + 1, name, valid, {1: "+", -1: "-", 0: "."}[strand], pos, pos + 1, "255,0,0", valid, pct, n_mod, n_canon, n_other,
                                                0, n_fail, 0, 0)) + "\n")
    return "".join(out).encode("latin-1")


def tsv_text(summary, cname, code_name, motifs):
    """PREFIX.motifs.tsv: the contigs' rows and the rows * (none for an empty summary)"""
    def line(name, j, k, sums):
        frac = "%.6f" % (sums[4] / sums[3]) if sums[3] else "NA"
        return "\t".join([name, motifs[j][0], str(motifs[j][1]), code_name[k]] + [str(x) for x in sums] + [frac]) + "\n"
    out, total = [TSV_HEADER], {}
    for c, j, k, *sums in summary:
        out.append(line(cname[c], j, k, sums))
        total[(j, k)] = [a + b for a, b in zip(total.get((j, k), [0] * 5), sums)]
    out += [line("*", j, k, total[(j, k)]) for (j, k) in sorted(total)]
    return "".join(out).encode("latin-1")
