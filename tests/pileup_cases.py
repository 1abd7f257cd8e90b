"""Jobs for the pileup's tests (metamaps_amd/csrc/mm_pileup_core.hpp on the host, mm_pileup_* on the device): the smallest shapes at which it can go
wrong.  A world is (contigs, jobs): job k's read is read k of the read set, its contig is contigs[job["c"]].  Jobs are pileup_ref.py's dicts."""
import numpy as np

import bam_cases
import edit_cases

I, D, EQ, X = bam_cases.I, bam_cases.D, bam_cases.EQ, bam_cases.X


def job(contigs, c, first, runs, strand=1, use=1, read=None):
    """a job on contig c whose read is made from the runs (bam_cases.job: = copies, X takes another base, I inserts G)"""
    j = bam_cases.job(b"p", contigs[c], first, runs, strand, read=read)
    return dict(read=j["read"], strand=strand, c=c, first=first, runs=j["runs"], d=j["d"], use=use)


def built_world():
    rng = np.random.default_rng(91)
    contigs = [edit_cases.dna(rng, 400), edit_cases.dna(rng, 300)]
    n0 = len(contigs[0])
    jobs = {}
    jobs["eq_only"] = job(contigs, 0, 17, [(40, EQ)])                                 # no event
    jobs["x_at_0"] = job(contigs, 0, 0, [(1, X), (10, EQ)])
    jobs["x_at_end"] = job(contigs, 0, n0 - 11, [(10, EQ), (1, X)], -1)
    jobs["lead_i"] = job(contigs, 0, 30, [(2, I), (10, EQ)])                          # anchored on first
    jobs["trail_i"] = job(contigs, 0, 30, [(10, EQ), (3, I)])                         # on the last base, 39
    jobs["i_at_len"] = job(contigs, 0, n0 - 10, [(10, EQ), (2, I)])                   # r == the contig's length: anchored on its last base
    jobs["only_i"] = job(contigs, 1, 5, [(4, I)])                                     # nothing but an insertion (last = first - 1)
    for n in (1, 63, 64, 65, 200):
        jobs[f"d{n}"] = job(contigs, 1, 3, [(5, EQ), (n, D), (5, EQ)], 1 if n % 2 else -1)
    q = bytearray(bam_cases.job(b"p", contigs[0], 100, [(3, EQ), (70, X), (4, EQ)])["read"])   # the oriented read; an N among the mismatches
    q[3 + 11] = ord("N"); q[3 + 66] = ord("n")
    jobs["x70_rev_n"] = job(contigs, 0, 100, [(3, EQ), (70, X), (4, EQ)], -1, read=edit_cases.stored(bytes(q), -1))
    jobs["x70_fwd"] = job(contigs, 1, 100, [(3, EQ), (70, X), (4, EQ)], 1)
    for n in (0, 1, 63, 64, 65, 129):                                                 # tiles of 64 runs
        runs = ([(1, EQ), (1, X), (1, EQ), (1, D), (2, EQ), (1, I)] * 22)[:n]
        jobs[f"runs{n}"] = job(contigs, n % 2, 7 + n, runs, -1 if n % 3 == 0 else 1)
    jobs["long_then_short"] = job(contigs, 0, 2, [(2, EQ), (90, D), (1, X), (66, X), (1, I), (3, EQ), (65, D), (2, X)])
    jobs["twice_a"] = job(contigs, 1, 50, [(4, EQ), (1, X), (4, EQ)])                  # the same key twice
    jobs["twice_b"] = dict(jobs["twice_a"])
    jobs["same_pos_c0"] = job(contigs, 0, 280, [(5, EQ), (1, D), (5, EQ)])             # the same position on two contigs
    jobs["same_pos_c1"] = job(contigs, 1, 280, [(5, EQ), (1, D), (5, EQ)])
    jobs["not_used"] = job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)], use=0)
    jobs["not_aligned"] = dict(job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)]), d=-1, runs=[], first=-1)
    jobs["empty_read"] = job(contigs, 0, 9, [], read=b"")
    return contigs, jobs


def random_world(n=200, seed=92):
    """reads made from the contigs through random runs, so that the rules hold; some not used, some not aligned, N and lower case among the read bytes"""
    rng = np.random.default_rng(seed)
    contigs = [edit_cases.dna(rng, 1500), edit_cases.dna(rng, 700), edit_cases.dna(rng, 90)]
    jobs = []
    for k in range(n):
        c = int(rng.integers(0, 3))
        runs, span = [], 0
        budget = int(rng.integers(1, min(len(contigs[c]), 600)))
        while True:
            op = int(rng.choice([EQ, EQ, EQ, X, D, I]))
            ln = int(rng.integers(1, 80 if op == EQ else 4)) if rng.random() < 0.95 else int(rng.integers(60, 140))
            if op != I and span + ln > budget:
                break
            runs.append((ln, op)); span += 0 if op == I else ln
        first = int(rng.integers(0, len(contigs[c]) - span + 1))
        strand = int(rng.choice([-1, 1]))
        j = bam_cases.job(b"p", contigs[c], first, runs, 1)
        q = bytearray(j["read"])
        for p in np.flatnonzero(rng.random(len(q)) < 0.03):
            q[p] = b"NRacgt"[int(rng.integers(0, 6))]
        jj = dict(read=edit_cases.stored(bytes(q), strand) if strand < 0 else bytes(q), strand=strand, c=c, first=first, runs=j["runs"], d=j["d"], use=int(k % 7 != 3))
        if k % 11 == 5:
            jj.update(d=-1, runs=[], first=-1)
        jobs.append(jj)
    return contigs, jobs


def broken_jobs(contigs):
    """(job, overrides of the call's arrays, rule): every rule mm_pileup_events applies (mm_bam_encode's 1, 2, 4, 5, 6)"""
    base = job(contigs, 0, 2, [(4, EQ), (1, X), (2, D), (3, EQ), (1, I), (2, EQ)])
    r = base["runs"]
    n0 = len(contigs[0])
    return [(base, dict(read=99), 1), (base, dict(read=-1), 1), (base, dict(contig=99), 1), (base, dict(contig=-1), 1),
            (base, dict(strand=0), 2), (base, dict(strand=2), 2),
            (base, dict(runs=[r[0], 1 << 4 | 0] + r[2:]), 4), (base, dict(runs=[r[0], 1 << 4 | 3] + r[2:]), 4), (base, dict(runs=[r[0], 0 << 4 | 8] + r[2:]), 4),
            (base, dict(runs=r[:-1] + [3 << 4 | 7]), 5), (base, dict(runs=r[:-1]), 5),
            (base, dict(first=-1), 6), (base, dict(first=n0 - 11), 6)]


def finish_worlds():
    """(name, clen, table {key: count}, intervals, min_count, min_frac): the edges of mm_pileup_finish"""
    import pileup_ref as R
    k = R.key
    out = []
    # a site on an interval's first and on its last base; touching, overlapping, nested and disjoint intervals; a contig (2) with intervals and no site
    iv = [(0, 0, 9), (0, 10, 19), (0, 30, 49), (0, 40, 59), (0, 35, 38), (0, 80, 80), (2, 5, 24), (2, 5, 24), (2, 100, 119), (3, 0, 6)]
    t = {k(0, 0, 1): 1, k(0, 9, 5): 1, k(0, 10, 6): 1, k(0, 40, 0): 2, k(0, 49, 2): 1, k(0, 38, 5): 3, k(0, 80, 4): 1, k(3, 6, 3): 1, k(3, 0, 6): 1}
    out.append(("edges", [100, 50, 120, 7], t, iv, 1, 0.0))
    out.append(("count_eq_min_count", [100, 50, 120, 7], t, iv, 2, 0.0))
    # depth 4: count 2 == 0.5 * 4 is kept, count 1 is not; depth 3 next to it: count 2 kept, 1 not
    iv2 = [(0, 10, 20)] * 4 + [(1, 0, 5)] * 3
    t2 = {k(0, 15, 1): 2, k(0, 15, 2): 1, k(0, 16, 5): 1, k(1, 2, 0): 2, k(1, 2, 3): 1}
    out.append(("frac_half", [30, 6], t2, iv2, 1, 0.5))
    out.append(("nothing", [30, 6], {}, [], 3, 0.2))
    out.append(("intervals_only", [30, 6], {}, iv2, 3, 0.2))
    return out
