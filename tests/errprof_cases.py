"""Jobs for the error profile's tests (metamaps_amd/csrc/mm_errprof_core.hpp on the host, mm_errprof_* on the device): the smallest shapes at which the walk
can go wrong.  A world is (contigs, jobs): job k's read is read k of the read set, its contig is contigs[job["c"]].  Jobs are errprof_ref.py's dicts."""
import numpy as np

import bam_cases
import edit_cases
import pileup_cases

I, D, EQ, X = bam_cases.I, bam_cases.D, bam_cases.EQ, bam_cases.X

# contig 2, written by hand: homopolymers of 70 G (at 20), 66 A (at 94), 5 T (at 0 and at the end), an N at 170 and a lower-case n at 176, then plain sequence
HP = b"TTTTT" + b"ACGTCATGCAGTCAC" + b"G" * 70 + b"TCTA" + b"A" * 66 + b"CATGCATCGA" + b"NACGTAnACGTACCA" + b"GGGG" + b"ACTGACTGACGT" * 4 + b"CAGTTTTT"


def ramp(m, step=7, at=3):
    """asymmetric qualities: no read looks the same from both ends"""
    return [(step * k + at) % 94 for k in range(m)]


def job(contigs, c, first, runs, strand=1, use=1, edit=None, qual=None):
    """a job on contig c whose oriented read is made from the runs (bam_cases.job: = copies, X takes another base, I inserts G); edit: {index in the oriented
    read: byte}; qual: None, "ramp", or the stored qualities"""
    j = bam_cases.job(b"e", contigs[c], first, runs, 1)
    q = bytearray(j["read"])
    for at, b in (edit or {}).items():
        q[at] = b
    read = edit_cases.stored(bytes(q), strand)
    return dict(read=read, strand=strand, c=c, first=first, runs=j["runs"], d=j["d"], use=use, qual=ramp(len(read)) if qual == "ramp" else qual)


def built_world():
    rng = np.random.default_rng(191)
    contigs = [edit_cases.dna(rng, 500), edit_cases.dna(rng, 300), HP]
    n0, n2 = len(contigs[0]), len(HP)
    shapes = {}
    shapes["one_eq"] = (0, 17, [(1, EQ)], None)
    for n in (63, 64, 65, 128, 129):                                 # tiles of 64 runs
        shapes[f"runs{n}"] = (n % 2, 5 + n, ([(1, EQ), (1, X), (2, EQ), (1, D), (2, EQ), (1, I)] * 22)[:n], None)
    for n in (64, 65):                                               # the all-lanes path of every op
        shapes[f"eq{n}"] = (0, 3, [(n, EQ)], None)
        shapes[f"x{n}"] = (1, 9, [(2, EQ), (n, X), (2, EQ)], None)
    for n in (63, 64, 65):                                           # the bin cap, and I and D runs by one lane and by all
        shapes[f"i{n}"] = (0, 40, [(4, EQ), (n, I), (4, EQ)], None)
        shapes[f"d{n}"] = (0, 40, [(4, EQ), (n, D), (4, EQ)], None)
        shapes[f"i{n}_in_g"] = (2, 25, [(5, EQ), (n, I), (5, EQ)], None)           # G inserted among the G: a homopolymer
        shapes[f"d{n}_of_g"] = (2, 18, [(4, EQ), (n, D), (4 + 65 - n, EQ)], None)  # deleted G with a G behind them (n < 70)
    shapes["i65_last_breaks"] = (2, 25, [(5, EQ), (65, I), (5, EQ)], {5 + 64: ord("T")})
    shapes["i64_first_breaks"] = (2, 25, [(5, EQ), (64, I), (5, EQ)], {5: ord("C")})
    shapes["i3_has_n"] = (2, 25, [(5, EQ), (3, I), (5, EQ)], {6: ord("N")})
    shapes["d70_whole_g"] = (2, 15, [(5, EQ), (70, D), (4, EQ)], None)               # all the G: no G on either side
    shapes["d66_whole_a"] = (2, 90, [(4, EQ), (66, D), (5, EQ)], None)
    shapes["d2_mixed"] = (2, 10, [(3, EQ), (2, D), (3, EQ)], None)
    shapes["i_g_before_g"] = (2, 15, [(5, EQ), (2, I), (5, EQ)], None)               # R[r] is the first G, R[r - 1] is not
    shapes["i_g_behind_g"] = (2, 85, [(5, EQ), (2, I), (5, EQ)], None)               # R[r - 1] is the last G, R[r] is not
    shapes["lead_i_at_0"] = (2, 0, [(2, I), (6, EQ)], {0: ord("T"), 1: ord("T")})    # r = 0: only R[0] can make it a homopolymer
    shapes["lead_i_at_0_other"] = (0, 0, [(3, I), (6, EQ)], None)
    shapes["d_at_0"] = (2, 0, [(3, D), (6, EQ)], None)                               # TTT of TTTTT deleted at position 0
    shapes["d_to_last_base"] = (2, n2 - 9, [(6, EQ), (3, D)], None)                  # r + n is the contig's length
    shapes["d_ends_before_last"] = (2, n2 - 9, [(5, EQ), (3, D), (1, EQ)], None)
    shapes["i_after_last_base"] = (2, n2 - 6, [(6, EQ), (2, I)], {6: ord("T"), 7: ord("T")})   # r is the contig's length
    shapes["i_after_last_other"] = (0, n0 - 6, [(6, EQ), (2, I)], None)
    shapes["only_i"] = (1, 5, [(4, I)], None)
    shapes["n_in_read_x"] = (0, 100, [(3, EQ), (5, X), (4, EQ)], {4: ord("N"), 6: ord("n")})
    shapes["n_in_ref_x"] = (2, 167, [(2, EQ), (5, X), (3, EQ)], None)                # 170 is N
    shapes["n_in_ref_x70"] = (2, 110, [(2, EQ), (70, X), (3, EQ)], None)              # 170 and 176 under a long run
    shapes["n_in_ref_d"] = (2, 165, [(3, EQ), (4, D), (10, EQ)], None)
    shapes["n_in_ref_eq"] = (2, 165, [(20, EQ)], None)                                # N against N, n against n: SUB[N][N]
    shapes["lower_case_read"] = (0, 200, [(6, EQ), (1, X), (6, EQ)], {0: ord("a"), 3: ord("r"), 6: ord("c")})
    shapes["long_then_short"] = (0, 2, [(2, EQ), (90, D), (1, X), (66, X), (1, I), (3, EQ), (65, D), (2, X), (70, I), (100, EQ)], None)
    jobs = {}
    for k, (name, (c, first, runs, edit)) in enumerate(shapes.items()):
        jobs[name + "_f"] = job(contigs, c, first, runs, 1, edit=edit, qual="ramp" if k % 2 else None)   # a set that mixes reads with and without qualities
        jobs[name + "_r"] = job(contigs, c, first, runs, -1, edit=edit, qual="ramp")
    jobs["q0"] = job(contigs, 0, 60, [(5, EQ), (2, X), (3, I), (5, EQ)], 1, qual=[0] * 15)
    jobs["q93"] = job(contigs, 0, 60, [(5, EQ), (2, X), (3, I), (5, EQ)], -1, qual=[93] * 15)
    jobs["q0_and_93"] = job(contigs, 0, 60, [(5, EQ), (2, X), (3, I), (5, EQ)], -1, qual=[0, 93] * 7 + [0])
    jobs["not_used"] = job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)], use=0, qual="ramp")
    jobs["not_aligned"] = dict(job(contigs, 0, 60, [(3, EQ), (2, X), (3, EQ)]), d=-1, runs=[], first=-1)
    jobs["empty_read"] = dict(job(contigs, 0, 9, []), read=b"")
    return contigs, jobs


def stutter(rng, n):
    """n bases in which homopolymers are common"""
    out = bytearray()
    while len(out) < n:
        out += bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.choice([1, 1, 1, 2, 3, 5, 8]))
    return bytes(out[:n])


def random_world(n=200, seed=192, max_columns=300):
    """reads made from stuttering contigs through random runs of at most max_columns columns in all, so that the rules hold; two thirds carry qualities, some
    jobs are not used or not aligned, N and lower case among the read bytes and inserted bases of every letter"""
    rng = np.random.default_rng(seed)
    contigs = [stutter(rng, 900), stutter(rng, 400), stutter(rng, 60)]
    jobs = []
    for k in range(n):
        c = int(rng.integers(0, 3))
        runs, span, columns = [], 0, 0
        budget = int(rng.integers(1, min(len(contigs[c]), max_columns)))
        while True:
            op = int(rng.choice([EQ, EQ, EQ, X, D, I]))
            ln = int(rng.integers(1, 40 if op == EQ else 4)) if rng.random() < 0.93 else int(rng.integers(60, 90))
            if columns + ln > budget:
                break
            runs.append((ln, op)); span += 0 if op == I else ln; columns += ln
        if not any(op != D for _, op in runs):
            runs.append((1, EQ)); span += 1
        first = int(rng.integers(0, len(contigs[c]) - span + 1))
        strand = int(rng.choice([-1, 1]))
        j = bam_cases.job(b"e", contigs[c], first, runs, 1)
        q = bytearray(j["read"])
        for p in np.flatnonzero(rng.random(len(q)) < 0.05):
            q[p] = b"NRacgtACGT"[int(rng.integers(0, 10))]
        qual = None if k % 3 == 0 else [int(v) for v in rng.integers(0, 94, size=len(q))]
        jj = dict(read=edit_cases.stored(bytes(q), strand), strand=strand, c=c, first=first, runs=j["runs"], d=j["d"], use=int(k % 7 != 3), qual=qual)
        if k % 11 == 5:
            jj.update(d=-1, runs=[], first=-1)
        jobs.append(jj)
    return contigs, jobs


def broken_jobs(contigs):
    """(job, overrides of the call's arrays, rule): mm_pileup_events' rules are mm_errprof_events'"""
    return pileup_cases.broken_jobs(contigs)


def finish_worlds():
    """(name, n_contigs, keys, cols): the ranks of 1 to 5 keys, equal keys, keys that do not count, a contig without any"""
    rng = np.random.default_rng(193)
    none = (1 << 64) - 1
    out = [("nothing", 3, [], []), ("only_skipped", 3, [none, none], [[1, 2, 3, 4, 5, 6]] * 2)]
    keys, cols = [], []
    for c, n in ((0, 1), (1, 2), (2, 3), (4, 4), (5, 5), (7, 9), (8, 64), (9, 65)):   # contigs 3 and 6 have none
        for k in range(n):
            keys.append(c << 32 | int(rng.integers(0, 1_000_001)))
            cols.append([int(v) for v in rng.integers(0, 5000, size=6)])
    keys += [none] * 3; cols += [[9, 9, 9, 9, 9, 9]] * 3
    keys += [6 << 32 | 1_000_000] * 3 + [6 << 32 | 0]; cols += [[100, 0, 0, 0, 0, 0]] * 3 + [[0, 50, 0, 0, 0, 0]]   # equal keys, and both ends of ppm
    out.append(("ranks", 11, keys, cols))
    order = rng.permutation(len(keys))
    out.append(("ranks_shuffled", 11, [keys[i] for i in order], [cols[i] for i in order]))
    out.append(("large_sums", 2, [1 << 32 | 999_999] * 3, [[2_000_000_000] * 6] * 3))   # the sums pass 2^32
    return out
