"""Cases for the base-modification tests (metamaps_amd/csrc/mm_mods_core.hpp on the host, mm_seqset_add_mods and mm_mod_* on the device): the smallest
shapes at which they can go wrong.  Groups and jobs are mods_ref.py's dicts; everything is seeded and built once per call."""
import numpy as np

import bam_cases
import edit_cases
import mods_ref

I, D, EQ, X = bam_cases.I, bam_cases.D, bam_cases.EQ, bam_cases.X
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 4097)
EDGE_ML = (0, 51, 52, 127, 128, 203, 204, 254, 255)                # around canonical/modified (127/128) and the thresholds 204 and 255, both ways (255 - 51 = 204)
CODE_BASE = "CCA"                                                  # the asked codes of the worlds below: C+m, C+h, A+a


def group(read, base, code, mode, at, ml):
    """the group that names the bases at the read indexes `at` (ascending, all of letter `base`) with the bytes ml"""
    letters = bytes(read).decode("latin-1").upper()
    assert all(letters[i] == base for i in at) and list(at) == sorted(set(at)) and len(at) == len(ml)
    ords = [letters[:i + 1].count(base) for i in at]
    return dict(base=base, code=code, mode=mode, skips=[o - p - 1 for o, p in zip(ords, [0] + ords[:-1])], ml=[int(x) for x in ml])


def _read_with(rng, n, base, at):
    r = bytearray(edit_cases.dna(rng, n))
    for i in at:
        r[i] = ord(base)
    return bytes(r)


def plane_cases():
    """[(name, read, groups, bad)]: bad is None, or the group mods_ref.plane must name in its DataError"""
    rng = np.random.default_rng(401)
    out = []
    for n in LENGTHS:
        at = sorted({i for i in (0, 63, 64, n - 1) if 0 <= i < n})
        read = _read_with(rng, n, "C", at)
        out.append((f"edges_{n}", read, [group(read, "C", 0, "?", at, [230 - 7 * k for k in range(len(at))])], None))       # the first and the last C are named
        allc = [i for i, ch in enumerate(read) if ch == ord("C")]
        g = group(read, "C", 0, "?", allc[-1:], [240] * len(allc[-1:]))                                                                       # ordinal == the count of C
        out.append((f"last_{n}", read, [g], None))
        out.append((f"beyond_{n}", read, [dict(g, skips=[len(allc)], ml=[240])], 0))                                           # count + 1
        out.append((f"beyond_second_group_{n}", read, [dict(g, skips=[], ml=[]), dict(g, base="G", code=1, skips=[read.count(b"G")], ml=[9])], 1))
    read = b"ACCGTCNcaCTAnC" * 6                                                                                             # lower case counts as its letter, N as none
    cs = [i for i, ch in enumerate(read.upper()) if ch == ord("C")]
    some = cs[1::3]
    for mode in (".", "?", ""):
        out.append((f"mode_{mode or 'absent'}", read, [group(read, "C", 0, mode, some, [250] * len(some))], None))
        out.append((f"empty_skips_{mode or 'absent'}", read, [dict(base="C", code=0, mode=mode, skips=[], ml=[])], None))
    for name, pm, ph in (("sum_255", 100, 155), ("sum_above_255", 200, 200), ("tie_to_canonical", 100, 55), ("equal_p_first", 120, 120), ("second_larger", 10, 200)):
        out.append((f"two_groups_{name}", read, [group(read, "C", 0, "?", some, [pm] * len(some)), group(read, "C", 1, "?", some, [ph] * len(some))], None))
    out.append(("two_groups_dot_and_ask", read, [group(read, "C", 0, ".", cs[::2], [210] * len(cs[::2])), group(read, "C", 1, "?", cs[::3], [190] * len(cs[::3]))], None))
    out.append(("unlisted_code", read, [group(read, "C", -1, "?", some, [222] * len(some)), group(read, "A", 2, ".", [0], [255])], None))
    out.append(("huge_skips", read, [dict(base="T", code=3, mode="?", skips=[0xFFFFFFFF] * 5, ml=[1, 2, 3, 4, 5])], 0))           # sums past 2^32: no wrap
    out.append(("no_groups", read, [], None))
    for k in range(12):                                                                                                       # random groups on random reads
        n = int(rng.integers(1, 700))
        read = edit_cases.sprinkle(rng, edit_cases.dna(rng, n), 0.05, b"NR")
        groups = []
        for base, code, mode in (("C", 0, "?"), ("C", 1, "?"), ("A", 2, "."), ("G", -1, ""), ("T", 3, "?"))[:int(rng.integers(1, 6))]:
            idx = [i for i, ch in enumerate(bytes(read).upper()) if ch == ord(base)]
            at = [i for i in idx if rng.random() < 0.5]
            groups.append(group(read, base, code, mode, at, rng.choice(EDGE_ML, size=len(at))))
        out.append((f"random_{k}", bytes(read), groups, None))
    return out


def dense_groups(rng, read):
    """C+m? and C+h? on the same C's (most of them), A+a. on half of the A's, G+other? on a few G's: every class comes out, and bytes at every edge"""
    up = bytes(read).upper()
    cs = [i for i, ch in enumerate(up) if ch == ord("C") and rng.random() < 0.8]
    a_ = [i for i, ch in enumerate(up) if ch == ord("A") and rng.random() < 0.5]
    gs = [i for i, ch in enumerate(up) if ch == ord("G") and rng.random() < 0.2]
    pm = rng.choice(EDGE_ML, size=len(cs))
    ph = np.where(rng.random(len(cs)) < 0.5, 0, np.minimum(255 - pm, rng.choice(EDGE_ML, size=len(cs))))
    return [group(read, "C", 0, "?", cs, pm), group(read, "C", 1, "?", cs, ph), group(read, "A", 2, ".", a_, rng.choice(EDGE_ML, size=len(a_))),
            group(read, "G", -1, "?", gs, [255] * len(gs))]


def job(rng, contigs, c, first, runs, strand=1, use=1, with_plane=True):
    j = bam_cases.job(b"m", contigs[c], first, runs, strand)
    groups = dense_groups(rng, j["read"]) if with_plane else None
    return dict(read=j["read"], strand=strand, c=c, first=first, runs=j["runs"], d=j["d"], use=use, groups=groups,
                plane=mods_ref.plane(j["read"], groups) if with_plane else None)


def event_world():
    """(contigs, {name: job}): = runs of 1, 63, 64, 65 and 200 with X, I and D between them and a leading insertion, on both strands; jobs that do not
    contribute; a read without a plane"""
    rng = np.random.default_rng(402)
    contigs = [edit_cases.dna(rng, 900), edit_cases.dna(rng, 500)]
    runs = [(2, I), (1, EQ), (1, X), (63, EQ), (2, D), (64, EQ), (1, I), (65, EQ), (3, X), (200, EQ)]
    jobs = {}
    jobs["fwd"] = job(rng, contigs, 0, 11, runs)
    jobs["rev"] = job(rng, contigs, 0, 300, runs, -1)
    jobs["rev_c1"] = job(rng, contigs, 1, 0, runs, -1)
    jobs["to_the_end"] = job(rng, contigs, 1, 500 - 70, [(70, EQ)])
    jobs["one_base"] = job(rng, contigs, 1, 77, [(1, EQ)])
    jobs["same_again"] = dict(jobs["fwd"])                                                # every key of `fwd` twice
    jobs["many_runs"] = job(rng, contigs, 0, 40, [(3, EQ), (1, X), (2, EQ), (1, D), (4, EQ), (1, I)] * 30, -1)   # three tiles of 64 runs
    jobs["no_eq"] = job(rng, contigs, 0, 5, [(4, X), (2, I)])
    jobs["not_used"] = job(rng, contigs, 0, 60, runs, use=0)
    jobs["not_aligned"] = dict(job(rng, contigs, 0, 60, runs), d=-1, runs=[], first=-1)
    jobs["no_plane"] = job(rng, contigs, 1, 20, runs, with_plane=False)
    return contigs, jobs


def random_world(n=40, seed=403):
    """about 40 jobs of 100 to 3 000 bases on three contigs, both strands, every fifth read without a plane"""
    rng = np.random.default_rng(seed)
    contigs = [edit_cases.dna(rng, 6000), edit_cases.dna(rng, 3500), edit_cases.dna(rng, 3100)]
    jobs = []
    for k in range(n):
        c = int(rng.integers(0, 3))
        runs, span, budget = [], 0, int(rng.integers(300, 3000))
        while True:
            op = int(rng.choice([EQ, EQ, EQ, X, D, I]))
            ln = int(rng.integers(1, 120 if op == EQ else 4))
            if op != I and span + ln > budget:
                break
            runs.append((ln, op)); span += 0 if op == I else ln
        first = int(rng.integers(0, len(contigs[c]) - span + 1))
        jobs.append(job(rng, contigs, c, first, runs, int(rng.choice([-1, 1])), use=int(k % 9 != 4), with_plane=k % 5 != 3))
    return contigs, jobs


def row_worlds():
    """[(name, contigs, table {key: count}, code_base, min_coverage)]: the edges of mm_mod_finish"""
    K = mods_ref.key
    contigs = [b"ACGTNacgtRCCGGAATT", b"CCAAGT"]
    t = {}
    for pos in range(len(contigs[0])):                                                   # every class on every byte, both strands: N, R and lower case among them
        for strand in (1, -1):
            for cls in range(6):
                t[K(0, pos, strand, cls)] = 1 + (pos * 7 + cls * 3 + (strand < 0)) % 5
    t[K(1, 0, 1, 3)] = 2; t[K(1, 0, 1, 4)] = 3; t[K(1, 0, 1, 0)] = 1                     # two listed codes on one C: each one's N_other holds the other
    t[K(1, 1, 1, 1)] = 9                                                                 # a segment of fail calls only: valid coverage 0
    t[K(1, 2, -1, 5)] = 4                                                                # A on the - strand is T: no code of base T
    t[K(1, 5, -1, 5)] = 4; t[K(1, 5, -1, 0)] = 1                                         # T on the - strand is A
    t[K(1, 4, -1, 3)] = 0xFFFFFFFF; t[K(1, 4, -1, 4)] = 0xFFFFFFFF; t[K(1, 4, -1, 2)] = 7   # sums past 32 bits
    out = [("all", contigs, t, CODE_BASE, 1), ("one_code", contigs, {k: v for k, v in t.items() if k & 7 < 4}, "C", 1), ("four_codes", contigs, {**t, K(1, 3, 1, 6): 2}, "CCAA", 1)]
    cov = {K(1, 0, 1, 0): 2, K(1, 0, 1, 3): 1, K(1, 0, 1, 1): 50, K(1, 1, 1, 0): 1, K(1, 1, 1, 4): 1, K(1, 1, 1, 1): 50}   # coverage 3 and 2, fail calls do not count
    out.append(("coverage_eq_min", contigs, cov, CODE_BASE, 3))
    out.append(("nothing", contigs, {}, CODE_BASE, 1))
    return out
