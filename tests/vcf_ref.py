"""The alleles of mapDirectly --vcf, restated plainly: strings, lists and dicts, an insertion carried as its letters and turned by slicing.  It shares no
code with metamaps_amd/csrc/mm_vcf_core.hpp or host/vcf_out.hpp; tests/test_vcf_core.py holds the header's host form to it, tests/test_gpu_vcf.py the
device, and tests/test_gpu_cli_vcf.py the file of the command line.

A job is pileup_ref.py's dict: read (the bytes its set holds), strand, c (the contig's index), first, runs (len << 4 | op words), d and use.  contigs
is the list of the reference's byte strings.  An allele is (contig, pos, kind, payload): ("S", letter), ("D", n) or ("I", letters)."""
import pileup_ref

NORM_MAX = 256
EXPLICIT_MAX = 24
WINDOW = 25
DEL, INS = 5, 6

contributes = pileup_ref.contributes
interval = pileup_ref.interval
depth = pileup_ref.depth


def ref_letters(contig):
    return bytes(contig).decode("latin-1").upper()


def alleles(j, contigs):
    """the normalised alleles of one contributing alignment, in the order of the walk"""
    q = pileup_ref.oriented(j["read"], j["strand"])
    ref = ref_letters(contigs[j["c"]])
    first, last = j["first"], interval(j)[2]
    r, i, out = first, 0, []
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op == 7:
            r += n; i += n
        elif op == 8:
            out += [(j["c"], r + t, "S", q[i + t]) for t in range(n) if q[i + t] != "N"]
            r += n; i += n
        elif op == 2:
            if first < r and r + n <= last:                         # an aligned reference position on both sides
                a = r - 1
                for _ in range(NORM_MAX):
                    if not (a > first and ref[a] in "ACGT" and ref[a] == ref[a + n]):
                        break
                    a -= 1
                out.append((j["c"], a, "D", n))
            r += n
        elif op == 1:
            s = "".join(q[i:i + n])
            if first < r <= last and "N" not in s:
                a = r - 1
                for _ in range(NORM_MAX):
                    if not (a > first and ref[a] in "ACGT" and ref[a] == s[-1]):
                        break
                    s = s[-1] + s[:-1]
                    a -= 1
                out.append((j["c"], a, "I", s))
            i += n
        else:
            raise ValueError(w)
    assert i == len(q)
    return out


def key(allele):
    """(w0, w1) of an allele"""
    c, pos, kind, x = allele
    if kind == "S":
        return c << 35 | pos << 3 | "ACGT".index(x), 0
    if kind == "D":
        assert 1 <= x < 1 << 16
        return c << 35 | pos << 3 | DEL, x
    assert 1 <= len(x) < 1 << 16
    bases = sum("ACGT".index(b) << 2 * k for k, b in enumerate(x)) if len(x) <= EXPLICIT_MAX else 0
    return c << 35 | pos << 3 | INS, len(x) << 48 | bases


def table(jobs, contigs):
    """{(w0, w1): count} over the contributing jobs"""
    t = {}
    for j in jobs:
        if contributes(j):
            for e in alleles(j, contigs):
                t[key(e)] = t.get(key(e), 0) + 1
    return t


def merged(triples):
    t = {}
    for a, b, c in triples:
        t[(int(a), int(b))] = t.get((int(a), int(b)), 0) + int(c)
    return t


def finish(t, intervals, contigs, min_count, min_frac):
    """[(w0, w1, count, depth, window)] in key order: the entries with count >= min_count and count >= min_frac * depth; window: WINDOW bytes of the
    upper-cased contig from the position on, zero bytes beyond its end"""
    out = []
    for k in sorted(t):
        c, pos = k[0] >> 35, (k[0] >> 3) & 0xFFFFFFFF
        d = depth(intervals, c, pos)
        if t[k] >= min_count and float(t[k]) >= min_frac * float(d):
            out.append((k[0], k[1], t[k], d, bytes(contigs[c]).upper()[pos:pos + WINDOW].ljust(WINDOW, b"\0")))
    return out


HEADER_TAIL = ('##INFO=<ID=DP,Number=1,Type=Integer,Description="Primary alignments that span the position">\n'
               '##INFO=<ID=AO,Number=1,Type=Integer,Description="Primary alignments that carry the allele">\n'
               '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of a symbolic allele">\n'
               '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Length of a symbolic allele, negative for a deletion">\n'
               '##INFO=<ID=END,Number=1,Type=Integer,Description="Last reference position of a symbolic allele">\n'
               '##ALT=<ID=INS,Description="Insertion of more than 24 bases">\n'
               '##ALT=<ID=DEL,Description="Deletion of more than 24 bases">\n'
               "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def header_text(cname, clen):
    return ("##fileformat=VCFv4.2\n##source=metamaps mapDirectly --vcf\n" + "".join(f"##contig=<ID={n},length={m}>\n" for n, m in zip(cname, clen)) + HEADER_TAIL).encode("latin-1")


def line(entry, cname):
    w0, w1, count, d, window = entry
    c, pos, code = w0 >> 35, (w0 >> 3) & 0xFFFFFFFF, w0 & 7
    ref = "".join(ch if ch in "ACGT" else "N" for ch in window.rstrip(b"\0").decode("latin-1"))
    info = f"DP={d};AO={count}"
    if code < 4:
        r, alt = ref[0], "ACGT"[code]
    elif code == DEL:
        n = w1
        if n <= EXPLICIT_MAX:
            r, alt = ref[:n + 1], ref[0]
            assert len(r) == n + 1
        else:
            r, alt, info = ref[0], "<DEL>", info + f";SVTYPE=DEL;SVLEN=-{n};END={pos + 1 + n}"
    else:
        assert code == INS
        n = w1 >> 48
        if n <= EXPLICIT_MAX:
            r, alt = ref[0], ref[0] + "".join("ACGT"[w1 >> 2 * k & 3] for k in range(n))
        else:
            r, alt, info = ref[0], "<INS>", info + f";SVTYPE=INS;SVLEN={n};END={pos + 1}"
    return f"{cname[c]}\t{pos + 1}\t.\t{r}\t{alt}\t.\t.\t{info}\n"


def vcf_text(entries, cname, clen):
    """PREFIX.vcf of finish()'s entries"""
    return header_text(cname, clen) + "".join(line(e, cname) for e in entries).encode("latin-1")
