"""Jobs with base qualities for the tests of the quality floor and of the BAM record's QUAL (tests/test_qual_core.py on the host, test_gpu_events_qual.py
on the device): the smallest shapes at which the floor can go wrong.  A world is (contigs, jobs); a job is qual_ref.py's dict: pileup_ref.py's with qual,
the stored Phred bytes of its read in read order, or None."""
import numpy as np

import bam_cases
import edit_cases
import pileup_cases

I, D, EQ, X = bam_cases.I, bam_cases.D, bam_cases.EQ, bam_cases.X
FLOOR = 20
HIGH, LOW = 40, FLOOR - 1


def with_qual(j, low=(), strand=None, high=HIGH, low_value=LOW):
    """the job with qualities `high` everywhere but `low_value` at the indexes `low` of the ORIENTED read"""
    m = len(j["read"])
    q = [high] * m
    for i in low:
        q[i] = low_value
    if (j["strand"] if strand is None else strand) < 0:
        q = q[::-1]
    return dict(j, qual=bytes(q))


def built_world():
    """{name: job}; the run under test starts at oriented read index 6 unless the name says otherwise"""
    rng = np.random.default_rng(311)
    c0 = bytearray(edit_cases.dna(rng, 900))
    c0[99:107] = b"AGGGGGGT"                                          # an insertion of G behind position 105 shifts left to 99
    contigs = [bytes(c0), edit_cases.dna(rng, 500)]
    job = lambda c, first, runs, strand=1: pileup_cases.job(contigs, c, first, runs, strand)
    jobs = {}
    # the floor's edge: q == Qm is kept, q == Qm - 1 is not
    jobs["x1_eq_floor"] = with_qual(job(0, 10, [(6, EQ), (1, X), (6, EQ)]), low=[6], low_value=FLOOR)
    jobs["x1_below"] = with_qual(job(0, 10, [(6, EQ), (1, X), (6, EQ)]), low=[6])
    # X and I runs of 1, 64, 65 and 200 (65 and 200: all lanes) with one low base first, at 63, at 64 and last
    for n in (1, 64, 65, 200):
        for at in sorted({0, 63, 64, n - 1}):
            if at >= n:
                continue
            for k, (op, name) in enumerate(((X, "x"), (I, "i"))):
                strand = -1 if (n + at + k) % 2 else 1
                jobs[f"{name}{n}_low{at}"] = with_qual(job(1, 20 + k, [(6, EQ), (n, op), (7, EQ)], strand), low=[6 + at])
        jobs[f"i{n}_high"] = with_qual(job(1, 30, [(6, EQ), (n, I), (7, EQ)]), low=[5, 6 + n])          # the bases around the insertion do not count
    # D runs: at i == 0 only q(0) is looked at, at i == m only q(m - 1); the calls accept such runs though the tracer never makes them
    jobs["d_at_0_low"] = with_qual(job(0, 40, [(3, D), (8, EQ)]), low=[0])
    jobs["d_at_0_kept"] = with_qual(job(0, 40, [(3, D), (8, EQ)]), low=[1])
    jobs["d_at_m_low"] = with_qual(job(0, 40, [(8, EQ), (3, D)]), low=[7])
    jobs["d_at_m_kept"] = with_qual(job(0, 40, [(8, EQ), (3, D)]), low=[6])
    jobs["d_left_low"] = with_qual(job(0, 200, [(6, EQ), (4, D), (6, EQ)]), low=[5])
    jobs["d_right_low"] = with_qual(job(0, 200, [(6, EQ), (4, D), (6, EQ)], -1), low=[6])
    jobs["d_kept"] = with_qual(job(0, 200, [(6, EQ), (4, D), (6, EQ)]), low=[4, 7])
    jobs["d70_left_low"] = with_qual(job(0, 300, [(6, EQ), (70, D), (6, EQ)], -1), low=[5])             # all lanes write one verdict
    jobs["d70_kept"] = with_qual(job(0, 300, [(6, EQ), (70, D), (6, EQ)]), low=[4])
    # strand -1: the low base is base 2 of the oriented read, stored at m - 3; read forward, the X base at 2 would be kept and the one at m - 3 dropped
    jobs["rev_low"] = with_qual(job(1, 60, [(2, EQ), (1, X), (6, EQ), (1, X), (2, EQ)], -1), low=[2])
    jobs["fwd_low"] = with_qual(job(1, 60, [(2, EQ), (1, X), (6, EQ), (1, X), (2, EQ)], 1), low=[2])
    # a read without qualities passes every floor
    jobs["no_qual"] = dict(job(1, 100, [(4, EQ), (2, X), (3, D), (4, EQ), (2, I), (4, EQ)]), qual=None)
    # an insertion that is dropped before its left shift, and a kept one that shifts as it does without a floor
    jobs["ins_shift_dropped"] = with_qual(job(0, 90, [(16, EQ), (2, I), (20, EQ)]), low=[17])
    jobs["ins_shift_kept"] = with_qual(job(0, 90, [(16, EQ), (2, I), (20, EQ)]), low=[15, 18])
    # tiles of 64 runs with a low base in the second tile
    runs = ([(1, EQ), (1, X), (1, EQ), (1, D), (2, EQ), (1, I)] * 22)[:129]
    m = sum(n for n, op in runs if op != D)
    jobs["runs129"] = with_qual(job(0, 400, runs, -1), low=range(m - 40, m, 3))
    return contigs, jobs


def random_world(n=200, seed=312):
    """reads of 50 to 3 000 bases made from two contigs through random runs, both strands, qualities 2 .. 40 drawn per base; every fifth read has none"""
    rng = np.random.default_rng(seed)
    contigs = [edit_cases.dna(rng, 4000), edit_cases.dna(rng, 3300)]
    jobs = []
    for k in range(n):
        c = int(rng.integers(0, 2))
        want = int(rng.integers(50, 3001))
        runs, span, m = [], 0, 0
        while m < want:
            op = int(rng.choice([EQ, EQ, EQ, X, D, I]))
            ln = int(rng.integers(1, 80 if op == EQ else 4)) if rng.random() < 0.95 else int(rng.integers(60, 140))
            if op != I and span + ln > len(contigs[c]):
                break
            runs.append((ln, op)); span += 0 if op == I else ln; m += 0 if op == D else ln
        first = int(rng.integers(0, len(contigs[c]) - span + 1))
        strand = int(rng.choice([-1, 1]))
        j = pileup_cases.job(contigs, c, first, runs, strand)
        q = bytearray(j["read"])
        for p in np.flatnonzero(rng.random(len(q)) < 0.02):
            q[p] = b"NRacgt"[int(rng.integers(0, 6))]
        j.update(read=bytes(q), use=int(k % 7 != 3), qual=None if k % 5 == 4 else rng.integers(2, 41, size=len(q)).astype(np.uint8).tobytes())
        if k % 11 == 5:
            j.update(d=-1, runs=[], first=-1)
        jobs.append(j)
    return contigs, jobs
