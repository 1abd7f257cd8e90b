"""Jobs for the tests of mapDirectly --vcf's alleles (metamaps_amd/csrc/mm_vcf_core.hpp on the host, mm_vcf_* on the device): the smallest shapes at which
they can go wrong.  A world is (contigs, jobs): job k's read is read k of the read set, its contig is contigs[job["c"]].  Jobs are pileup_ref.py's dicts."""
import numpy as np

import edit_cases

I, D, EQ, X = 1, 2, 7, 8


def other(b):
    return ord("C") if chr(b).upper() == "A" else ord("A")


def job(contigs, c, first, runs, strand=1, use=1):
    """a job on contig c whose oriented read is made from the runs: (n, EQ) copies the contig, (n, X) takes another base, (n, I) inserts G; (n, X, bases)
    and (n, I, bases) take the bases given"""
    ref, out, p, words = contigs[c], bytearray(), first, []
    for run in runs:
        n, op = run[0], run[1]
        if op == EQ:
            out += ref[p:p + n]
        elif op == X:
            out += run[2] if len(run) > 2 else bytes(other(b) for b in ref[p:p + n])
        elif op == I:
            out += run[2] if len(run) > 2 else b"G" * n
        if op != I:
            p += n
        assert len(run) < 3 or len(run[2]) == n
        words.append(n << 4 | op)
    assert 0 <= first and p <= len(ref)
    return dict(read=edit_cases.stored(bytes(out), strand), strand=strand, c=c, first=first, runs=words, d=sum(r[0] for r in runs if r[1] != EQ), use=use)


# where the built contigs carry planted sequence (contig, start)
HP12, DI10, TRI8, HAND, HP_N, HP300 = (0, 100), (0, 150), (0, 200), (0, 250), (0, 300), (1, 20)


def built_contigs():
    rng = np.random.default_rng(191)
    c0, c1 = bytearray(edit_cases.dna(rng, 600)), bytearray(edit_cases.dna(rng, 500))
    c0[0:6] = b"TTTTTT"                                            # a homopolymer at position 0
    c0[99:113] = b"C" + b"A" * 12 + b"G"
    c0[149:171] = b"T" + b"CA" * 10 + b"T"
    c0[199:225] = b"T" + b"CAG" * 8 + b"T"
    c0[250:257] = b"GACACAT"
    c0[299:311] = b"C" + b"A" * 4 + b"N" + b"A" * 5 + b"G"          # N at 304
    c1[19:321] = b"C" + b"A" * 300 + b"G"
    return [bytes(c0), bytes(c1)]


def built_world():
    contigs = built_contigs()
    n0 = len(contigs[0])
    shapes = {}
    shapes["eq_only"] = (0, 17, [(40, EQ)])
    shapes["lead_i"] = (0, 30, [(2, I), (10, EQ)])
    shapes["trail_i"] = (0, 30, [(10, EQ), (3, I)])
    shapes["lead_d"] = (0, 30, [(2, D), (10, EQ)])
    shapes["trail_d"] = (0, 30, [(10, EQ), (3, D)])
    shapes["lead_i_then_d"] = (0, 30, [(2, I), (3, D), (10, EQ)])  # the deletion is no first run, but no aligned base lies before it
    shapes["d_then_trail_i"] = (0, 30, [(10, EQ), (3, D), (2, I)])
    shapes["only_i"] = (1, 5, [(4, I)])
    shapes["x_at_0"] = (0, 0, [(1, X), (10, EQ)])
    shapes["x_at_end"] = (0, n0 - 11, [(10, EQ), (1, X)])
    shapes["hp_to_first_d"] = (0, HP12[1] + 2, [(6, EQ), (1, D), (20, EQ)])        # shifts to `first` and stops
    shapes["hp_to_first_i"] = (0, HP12[1] + 3, [(5, EQ), (2, I, b"AA"), (20, EQ)])
    shapes["hp_whole_d"] = (0, 90, [(18, EQ), (2, D), (20, EQ)])                   # stops at the C before the homopolymer: anchor 99
    shapes["at_0_d"] = (0, 0, [(3, EQ), (1, D), (20, EQ)])                          # first = 0: stops at position 0
    shapes["at_0_i"] = (0, 0, [(4, EQ), (1, I, b"T"), (20, EQ)])
    shapes["n_stops_d"] = (0, 295, [(13, EQ), (1, D), (20, EQ)])                    # r = 308 inside the second half: stops behind the N at 304
    shapes["n_stops_i"] = (0, 295, [(13, EQ), (1, I, b"A"), (20, EQ)])
    shapes["di_ins_1_5"] = (0, 140, [(26, EQ), (3, I, b"ACA"), (20, EQ)])           # r = 166 inside (CA)10
    shapes["tri_ins_1_5"] = (0, 190, [(28, EQ), (5, I, b"AGCAG"), (20, EQ)])        # r = 218 behind a whole CAG
    shapes["tri_del_1"] = (0, 190, [(25, EQ), (3, D), (20, EQ)])
    shapes["hand_rot"] = (0, 240, [(14, EQ), (2, I, b"CA"), (20, EQ)])              # GACA|CA|CAT: three shifts of two bases: AC behind the G at 250
    for k in (255, 256, 257):                                       # the steps the homopolymer of 300 leaves from `first`
        shapes[f"steps{k}_d"] = (1, 25, [(k + 1, EQ), (1, D), (20, EQ)])
        shapes[f"steps{k}_i"] = (1, 25, [(k + 1, EQ), (2, I, b"AA"), (20, EQ)])
    for n in (24, 25):
        shapes[f"d{n}"] = (1, 330, [(5, EQ), (n, D), (5, EQ)])
        shapes[f"i{n}"] = (1, 330, [(5, EQ), (n, I, (b"ACGTTGCA" * 4)[:n]), (5, EQ)])
    shapes["i_with_n"] = (0, 400, [(5, EQ), (3, I, b"ANA"), (5, EQ)])
    shapes["x_n_between"] = (0, 400, [(5, EQ), (3, X, b"GNg"), (5, EQ)])
    for n in (64, 65):
        shapes[f"x{n}"] = (0, 420, [(3, EQ), (n, X), (4, EQ)])
    shapes["x70_n"] = (1, 350, [(3, EQ), (70, X, bytes(ord("N") if t in (11, 66) else ord("T") for t in range(70))), (4, EQ)])
    for n in (63, 64, 65, 129):                                     # tiles of 64 runs
        runs = ([(1, EQ), (1, X), (1, EQ), (1, D), (2, EQ), (1, I)] * 22)[:n]
        shapes[f"runs{n}"] = (n % 2, 7 + n, runs)
    shapes["long_then_short"] = (0, 330, [(2, EQ), (90, D), (1, X), (66, X), (1, I), (3, EQ), (65, D), (2, X), (2, EQ)])
    jobs = {}
    for name, (c, first, runs) in shapes.items():
        for tag, strand in (("f", 1), ("r", -1)):
            jobs[f"{name}_{tag}"] = job(contigs, c, first, runs, strand)
    # the same deletion of one A of the homopolymer of 12, placed at its end by one read and in its middle by the other
    jobs["same_del_a"] = job(contigs, 0, 80, [(31, EQ), (1, D), (20, EQ)])           # r = 111: the last A
    jobs["same_del_b"] = job(contigs, 0, 85, [(20, EQ), (1, D), (20, EQ)], -1)       # r = 105
    jobs["not_used"] = job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)], use=0)
    jobs["not_aligned"] = dict(job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)]), d=-1, runs=[], first=-1)
    jobs["empty_read"] = job(contigs, 0, 9, [])
    return contigs, jobs


def random_world(n=200, seed=192, max_span=600):
    """reads made from low-complexity contigs through random runs, so that the rules hold and indels shift; some not used, some not aligned, N and lower case
    among the read bytes, N and IUPAC among the reference's"""
    rng = np.random.default_rng(seed)
    contigs = []
    for length in (1500, 700):
        s = bytearray()
        while len(s) < length:
            kind = int(rng.integers(0, 4))
            if kind == 0:
                s += edit_cases.dna(rng, int(rng.integers(5, 40)))
            elif kind == 1:
                s += bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(3, 30))
            elif kind == 2:
                s += edit_cases.dna(rng, int(rng.integers(2, 5))) * int(rng.integers(2, 12))
            else:
                s += bytes([b"NRn"[int(rng.integers(0, 3))]])
        contigs.append(bytes(s[:length]))
    contigs[1] = contigs[1][:300] + b"G" * 300 + contigs[1][600:]     # room for more than NORM_MAX shifts
    jobs = []
    for k in range(n):
        c = int(rng.integers(0, 2))
        runs, span = [], 0
        budget = int(rng.integers(1, min(len(contigs[c]), max_span)))
        while True:
            op = int(rng.choice([EQ, EQ, EQ, X, D, I]))
            ln = int(rng.integers(1, 80 if op == EQ else 4)) if rng.random() < 0.95 else int(rng.integers(20, 140))
            if op != I and span + ln > budget:
                break
            if op in (X, I):
                bases = bytearray(edit_cases.dna(rng, ln))
                if rng.random() < 0.25:                             # an N or a lower-case base somewhere in the run
                    bases[int(rng.integers(0, ln))] = b"Nna"[int(rng.integers(0, 3))]
                runs.append((ln, op, bytes(bases)))
            else:
                runs.append((ln, op))
            span += 0 if op == I else ln
        first = int(rng.integers(0, len(contigs[c]) - span + 1))
        jj = job(contigs, c, first, runs, int(rng.choice([-1, 1])), use=int(k % 7 != 3))
        if k % 11 == 5:
            jj.update(d=-1, runs=[], first=-1)
        jobs.append(jj)
    return contigs, jobs


def broken_jobs(contigs):
    """(job, overrides of the call's arrays, rule): every rule mm_vcf_events applies (mm_bam_encode's 1, 2, 4, 5, 6, and 8: an indel of 2^16 bases between
    other runs); contigs[2] has room for that run"""
    base = job(contigs, 0, 2, [(4, EQ), (1, X), (2, D), (3, EQ), (1, I), (2, EQ)])
    r = base["runs"]
    n0 = len(contigs[0])
    big = job(contigs, 2, 1, [(2, EQ), (65536, D), (2, EQ)])
    return [(base, dict(read=99), 1), (base, dict(read=-1), 1), (base, dict(contig=99), 1), (base, dict(contig=-1), 1),
            (base, dict(strand=0), 2), (base, dict(strand=2), 2),
            (base, dict(runs=[r[0], 1 << 4 | 0] + r[2:]), 4), (base, dict(runs=[r[0], 1 << 4 | 3] + r[2:]), 4), (base, dict(runs=[r[0], 0 << 4 | 8] + r[2:]), 4),
            (base, dict(runs=r[:-1] + [3 << 4 | 7]), 5), (base, dict(runs=r[:-1]), 5),
            (base, dict(first=-1), 6), (base, dict(first=n0 - 11), 6),
            (big, dict(), 8)]


def big_contig():
    """a contig with room for an indel run of 2^16 bases"""
    return edit_cases.dna(np.random.default_rng(193), 65600)


def finish_worlds():
    """(name, contigs, table {(w0, w1): count}, intervals, min_count, min_frac): the edges of mm_vcf_finish"""
    rng = np.random.default_rng(194)
    contigs = [bytearray(edit_cases.dna(rng, 100)), bytearray(edit_cases.dna(rng, 30))]
    contigs[0][9] = ord("N"); contigs[0][41] = ord("r"); contigs[1][28] = ord("n")
    contigs = [bytes(c) for c in contigs]

    def k(c, pos, code, w1=0):
        return (c << 35 | pos << 3 | code, w1)
    out = []
    # an anchor equal to an interval's first and to its last base; count == depth; the window clipped at each contig's end (and of one byte)
    iv = [(0, 10, 19), (0, 10, 29), (0, 40, 99), (0, 76, 99), (1, 0, 29), (1, 5, 29)]
    t = {k(0, 10, 5, 3): 2, k(0, 19, 6, 2 << 48 | 0b0110): 2, k(0, 29, 1): 1, k(0, 40, 2): 1, k(0, 40, 6, 30 << 48): 1, k(0, 41, 5, 24): 1, k(0, 41, 5, 25): 1, k(0, 76, 5, 23): 2,
         k(0, 99, 0): 2, k(1, 0, 3): 1, k(1, 4, 5, 25): 1, k(1, 5, 5, 24): 2, k(1, 6, 5, 5): 2, k(1, 6, 6, 1 << 48 | 3): 1, k(1, 28, 6, 1 << 48): 2, k(1, 29, 2): 2}
    out.append(("edges", contigs, t, iv, 1, 0.0))
    out.append(("count_eq_min_count", contigs, t, iv, 2, 0.0))
    # depth 4: count 2 == 0.5 * 4 is kept, count 1 is not; depth 3 next to it: count 2 kept, 1 not
    iv2 = [(0, 10, 20)] * 4 + [(1, 0, 5)] * 3
    t2 = {k(0, 15, 1): 2, k(0, 15, 5, 2): 1, k(0, 15, 5, 3): 2, k(0, 16, 6, 1 << 48 | 2): 1, k(1, 2, 0): 2, k(1, 2, 6, 40 << 48): 1}
    out.append(("frac_half", contigs, t2, iv2, 1, 0.5))
    out.append(("nothing", contigs, {}, [], 3, 0.2))
    out.append(("intervals_only", contigs, {}, iv2, 3, 0.2))
    return out
