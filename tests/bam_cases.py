"""Jobs for the BAM encoder's tests (metamaps_amd/csrc/mm_bam_core.hpp on the host, mm_bam_encode on the device): the smallest shapes at which it
can go wrong.  A job is a dict with name, read (as the set stores it), strand, contig (its bytes), first, runs, d, flag and mapq; job k's read is
read k of its set and its contig is contig k, so refID is k."""
import numpy as np

import edit_cases
import edit_cigar_ref
import edit_ref

I, D, EQ, X = 1, 2, 7, 8


def job(name, contig, first, runs, strand=1, read=None, mapq=17, secondary=False):
    """a job whose read is made from the runs: = copies the contig, X takes another base, I inserts G"""
    if read is None:
        out, j = bytearray(), first
        for n, op in runs:
            if op == EQ:
                out += contig[j:j + n]
            elif op == X:
                out += bytes(ord("C") if chr(b).upper() == "A" else ord("A") for b in contig[j:j + n])
            elif op == I:
                out += b"G" * n
            if op != I:
                j += n
        read = edit_cases.stored(bytes(out), strand)
    return dict(name=name, read=bytes(read), strand=strand, contig=bytes(contig), first=first, runs=[n << 4 | op for n, op in runs],
                d=sum(n for n, op in runs if op != EQ), flag=(0x10 if strand < 0 else 0) | (0x100 if secondary else 0), mapq=mapq)


def built_jobs():
    rng = np.random.default_rng(71)
    ref = edit_cases.dna(rng, 2600)
    out = []
    for m in (1, 2, 15, 16, 17, 31, 32, 33):                        # nibble and packed-word edges
        for strand in (1, -1):
            out.append(job(b"len%d%s" % (m, b"f" if strand > 0 else b"r"), ref[:100], 5, [(m, EQ)], strand))
    for k, ln in enumerate((1, 2, 3, 4, 254, 1, 3, 2, 4)):           # names: with the reads above, records start at every residue mod 4
        out.append(job(bytes([ord("a") + k]) * ln, ref[:64], k, [(7 + k, EQ)], 1, secondary=k % 2 == 1))
    out.append(job(b"iupac", ref[:40], 3, [(11, EQ)], -1, read=b"ACGTNRXacgy"))   # R becomes Y, X becomes N
    out.append(job(b"exact", ref[:400], 50, [(300, EQ)]))                        # MD 300
    out.append(job(b"xx", ref[:100], 1, [(5, EQ), (2, X), (6, EQ), (3, X), (4, EQ)]))
    out.append(job(b"xd_dx", ref[:100], 2, [(5, EQ), (1, X), (2, D), (7, EQ), (3, D), (1, X), (4, EQ)], -1))
    out.append(job(b"eq_i_eq", ref[:100], 0, [(5, EQ), (2, I), (3, EQ)]))          # MD 8
    out.append(job(b"counters", ref, 10, [(9, EQ), (1, X), (10, EQ), (1, X), (99, EQ), (1, X), (100, EQ), (1, X), (999, EQ), (1, X), (1000, EQ)]))
    dirty = bytearray(ref[:120]); dirty[20] = ord("N"); dirty[41] = ord("n"); dirty[60] = ord("-"); dirty[80] = ord("-"); dirty[81] = ord("r")
    out.append(job(b"ref_n", dirty, 10, [(10, EQ), (1, X), (19, EQ), (3, D), (17, EQ), (1, X), (18, EQ), (3, D), (9, EQ)]))
    out.append(job(b"d150", ref[:400], 7, [(40, EQ), (150, D), (40, EQ)]))
    big = edit_cases.dna(rng, 131080)
    out.append(job(b"bin4681", big[:16400], 16383, [(1, EQ)]))
    out.append(job(b"bin585", big[:16400], 16383, [(2, EQ)]))
    out.append(job(b"bin73", big, 131071, [(2, EQ)]))                              # crosses 2^17: the level of 2^20
    out.append(job(b"bin9", edit_cases.dna(rng, 1048580), 1048575, [(2, EQ)]))     # crosses 2^20: the level of 2^23
    out.append(job(b"runs70000", big[:70010], 3, [(1, EQ), (1, X)] * 35000, -1))   # the CG tag
    out.append(job(b"runs65535", big[:65600], 0, ([(1, EQ), (1, X)] * 32768)[:65535]))
    out.append(job(b"runs65536", big[:65600], 1, [(1, X), (1, EQ)] * 32768))
    return out


def random_jobs(n=200, seed=72, max_len=400):
    """reads of 1 to max_len bases planted in windows, both strands, aligned by the reference aligner; the ones it does not align are left out"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        m = int(rng.integers(1, max_len + 1))
        read, strand, win = edit_cases.planted(rng, m, int(rng.integers(0, 30)), int(rng.integers(0, 30)), float(rng.choice([0.0, 0.05, 0.15])),
                                               int(rng.choice([-1, 1])), 0.04 if len(out) % 4 == 0 else 0.0)
        got = edit_cigar_ref.align(read, strand, win, edit_ref.cap(len(read), 70.0))
        if got is None or len(read) == 0:
            continue
        d, a, b, runs = got
        k = len(out)
        out.append(dict(name=b"r%d" % k + b"x" * (k % 5), read=read, strand=strand, contig=win, first=a, runs=runs, d=d,
                        flag=(0x10 if strand < 0 else 0) | (0x100 if k % 3 == 0 else 0), mapq=k % 61))
    return out


def broken_jobs():
    """(job, overrides of the call's arrays, rule): every rule of mm_bam_encode"""
    base = job(b"ok", b"ACGTACGTACGTACGTACGT", 2, [(4, EQ), (1, X), (2, D), (3, EQ), (1, I), (2, EQ)])
    r = base["runs"]
    return [(base, dict(read=1), 1), (base, dict(read=-1), 1), (base, dict(contig=1), 1), (base, dict(contig=-1), 1),
            (base, dict(strand=0), 2), (base, dict(strand=2), 2), (base, dict(flag=0x10), 2), (base, dict(strand=-1), 2),
            (base, dict(name=b""), 3), (base, dict(name=b"n" * 255), 3),
            (base, dict(runs=[r[0], 1 << 4 | 0] + r[2:]), 4), (base, dict(runs=[r[0], 1 << 4 | 3] + r[2:]), 4), (base, dict(runs=[r[0], 0 << 4 | 8] + r[2:]), 4),
            (base, dict(runs=r[:-1] + [3 << 4 | 7]), 5), (base, dict(runs=r[:-1]), 5),
            (base, dict(first=-1), 6), (base, dict(first=9), 6),
            (base, dict(d=3), 7), (base, dict(d=5), 7)]


def record_of(bam_ref, j, k):
    return bam_ref.record(j["name"], j["read"], j["strand"], k, j["contig"], j["first"], j["runs"], j["d"], j["flag"], j["mapq"])
