"""Base qualities restated plainly: the QUAL field of a BAM record and the quality floor of mm_pileup_events_q / mm_vcf_events_q (mapDirectly
--min-base-quality).  It shares no code with metamaps_amd/csrc/mm_pileup_core.hpp or mm_vcf_core.hpp; tests/test_qual_core.py holds the headers' host form
to it, tests/test_gpu_events_qual.py and test_gpu_bam_qual.py the device.

A job is pileup_ref.py's dict with one more entry: qual, the stored Phred bytes of its read in read order (as long as read), or None for a read without
qualities.  "No quality" counts as 255 and passes every floor."""
import pileup_ref
import vcf_ref

NONE = 255


def oriented(j):
    """the quality of every base of the read as it is aligned"""
    m = len(j["read"])
    q = [NONE] * m if j.get("qual") is None else list(bytes(j["qual"]))
    assert len(q) == m
    return q[::-1] if j["strand"] < 0 else q


def bam_qual(j):
    """QUAL of the job's BAM record"""
    return bytes(oriented(j))


def _del_kept(q, i, floor):
    """a D run met at read index i: the read's bases on either side of the gap"""
    side = ([q[i - 1]] if i > 0 else []) + ([q[i]] if i < len(q) else [])
    return min(side, default=NONE) >= floor


def events(j, floor):
    """pileup_ref.events(j) under the floor"""
    q = oriented(j)
    r, i, out = j["first"], 0, []
    base = pileup_ref.oriented(j["read"], j["strand"])
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op == 7:
            r += n; i += n
        elif op == 8:
            out += [(j["c"], r + t, "ACGTN".index(base[i + t])) for t in range(n) if q[i + t] >= floor]
            r += n; i += n
        elif op == 2:
            if _del_kept(q, i, floor):
                out += [(j["c"], r + t, pileup_ref.DEL) for t in range(n)]
            r += n
        elif op == 1:
            if min(q[i:i + n]) >= floor:
                out.append((j["c"], r - 1 if r > j["first"] else j["first"], pileup_ref.INS))
            i += n
        else:
            raise ValueError(w)
    assert i == len(q)
    return out


def table(jobs, floor):
    """{key: count} over the contributing jobs"""
    t = {}
    for j in jobs:
        if pileup_ref.contributes(j):
            for e in events(j, floor):
                t[pileup_ref.key(*e)] = t.get(pileup_ref.key(*e), 0) + 1
    return t


def alleles(j, contigs, floor):
    """vcf_ref.alleles(j, contigs) under the floor: a run that is not kept gives no allele, and is asked before the shift"""
    q = oriented(j)
    base = pileup_ref.oriented(j["read"], j["strand"])
    ref = vcf_ref.ref_letters(contigs[j["c"]])
    first, last = j["first"], pileup_ref.interval(j)[2]
    r, i, out = first, 0, []
    for w in j["runs"]:
        n, op = int(w) >> 4, int(w) & 15
        if op == 7:
            r += n; i += n
        elif op == 8:
            out += [(j["c"], r + t, "S", base[i + t]) for t in range(n) if base[i + t] != "N" and q[i + t] >= floor]
            r += n; i += n
        elif op == 2:
            if first < r and r + n <= last and _del_kept(q, i, floor):
                a = r - 1
                for _ in range(vcf_ref.NORM_MAX):
                    if not (a > first and ref[a] in "ACGT" and ref[a] == ref[a + n]):
                        break
                    a -= 1
                out.append((j["c"], a, "D", n))
            r += n
        elif op == 1:
            s = "".join(base[i:i + n])
            if first < r <= last and "N" not in s and min(q[i:i + n]) >= floor:
                a = r - 1
                for _ in range(vcf_ref.NORM_MAX):
                    if not (a > first and ref[a] in "ACGT" and ref[a] == s[-1]):
                        break
                    s = s[-1] + s[:-1]
                    a -= 1
                out.append((j["c"], a, "I", s))
            i += n
        else:
            raise ValueError(w)
    return out


def vcf_table(jobs, contigs, floor):
    """{(w0, w1): count} over the contributing jobs"""
    t = {}
    for j in jobs:
        if pileup_ref.contributes(j):
            for e in alleles(j, contigs, floor):
                t[vcf_ref.key(e)] = t.get(vcf_ref.key(e), 0) + 1
    return t
