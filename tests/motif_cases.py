"""Worlds for the tests of mapDirectly --mod-motifs (metamaps_amd/csrc/mm_motif_core.hpp on the host, mm_mod_motifs on the device): the smallest shapes at which
the scan and the sites' kernel can still go wrong.  A case is a dict: name, contigs (upper-case bytes), table ({key: count}, mods_ref.key), code_base, motifs
[(letters, offset)], min_coverage, min_frac, combine, and check(rows, summary), which says whether motif_ref.profile's answer shows what the case is named for
(test_motif_core.py asserts it for every case).  Built on the CPU."""
import numpy as np

import mods_ref
import motif_ref

TILE = 2048                                                        # mmt::SCAN_TILE (tests/test_motif_core.cpp prints the header's)
K = mods_ref.key


def _case(name, contigs, table, code_base, motifs, check, min_coverage=1, min_frac=0.5, combine=False):
    return dict(name=name, contigs=contigs, table=table, code_base=code_base, motifs=motifs, min_coverage=min_coverage, min_frac=min_frac, combine=combine, check=check)


def _sites(summary):
    return {(c, j, k): s[0] for c, j, k, *s in summary}


def _ends():
    a, b, c = b"GATCTTTTTTGATC", b"T" * 14 + b"GA", b"TCTTTTTTGAT"        # b fills its 16 stream positions: GA and TC are neighbours in the stream
    t = {K(0, 1, 1, 3): 2, K(0, 11, 1, 0): 1, K(0, 2, -1, 3): 1, K(1, 15, 1, 0): 1, K(2, 0, -1, 0): 1}
    # first and last start of contig 0 on both strands; nothing across b|c, nothing for the GAT that c's end cuts
    return _case("ends_and_boundary", [a, b, c], t, "A", [("GATC", 1)], lambda rows, s: _sites(s) == {(0, 0, 0): 4, (1, 0, 0): 0, (2, 0, 0): 0} and len(rows) == 3)


def _tile_boundary():
    rng = np.random.default_rng(71)
    contigs, t, starts = [], {}, set()
    for k in range(5):                                             # starts TILE - 40 .. TILE + 40, those equal to k mod 5 in contig k (a plant has 5 letters)
        seq = bytearray(b"T" * (3 * TILE))                         # (a multiple of 16: contig k starts at tile 3k of the stream)
        for s in range(TILE - 40, TILE + 41):
            if s % 5 == k:
                seq[s:s + 5] = b"GA" + bytes([b"ACGT"[int(rng.integers(0, 4))]]) + b"TC"
                starts.add(s)
                t[K(k, s + 1, 1, 3)] = 1 + s % 3
                if s % 2:
                    t[K(k, s + 3, -1, 0)] = 2
        contigs.append(bytes(seq))
    assert starts == set(range(TILE - 40, TILE + 41))
    n = sum(1 for s in starts if s % 2)
    return _case("three_tiles_boundary", contigs, t, "A", [("GANTC", 1)],
                 lambda rows, s: sum(_sites(s).values()) == 2 * 81 and len(rows) == 81 + n and {r[1] for r in rows if r[2] > 0} == {x + 1 for x in starts})


def _small():
    """three contigs inside one tile; overlapping occurrences; two motifs on one site; two codes of one base beside a code of another motif's base"""
    contigs = [b"TTAAAAAATT", b"TTCGCGCGTT", b"TTCCGGTTACGT"]
    t = {K(0, 2, 1, 5): 3, K(0, 6, 1, 0): 1, K(0, 7, 1, 5): 1, K(0, 9, -1, 5): 2, K(0, 8, -1, 0): 1,
         K(1, 2, 1, 3): 2, K(1, 2, 1, 4): 3, K(1, 2, 1, 0): 1, K(1, 2, 1, 2): 1, K(1, 2, 1, 1): 4, K(1, 4, 1, 4): 1, K(1, 7, -1, 3): 5,
         K(2, 3, 1, 3): 1, K(2, 3, 1, 0): 1, K(2, 4, -1, 4): 2, K(2, 9, 1, 0): 7, K(2, 8, 1, 5): 1}
    motifs = [("AA", 0), ("CG", 0), ("CCGG", 1)]

    def check(rows, s):
        at = {(r[0], r[1], r[2], r[3], r[4]): r[5:] for r in rows}
        return (_sites(s)[(0, 0, 2)] == 5 + 2 and _sites(s)[(1, 1, 0)] == 6                  # AA in A6 (+) and in TT, TT (-); CG in CGCGCG both strands
                and at[(1, 2, 1, 1, 0)] == (2, 1, 4, 4) and at[(1, 2, 1, 1, 1)] == (3, 1, 3, 4)    # each C code's N_other holds the other
                and (2, 3, 1, 1, 0) in at and (2, 3, 1, 2, 0) in at                              # CG:0 and CCGG:1 share the site
                and not any(r[4] == 2 and r[3] != 0 for r in rows))                              # the A code belongs to AA:0 alone
    return _case("three_contigs_one_tile", contigs, t, "CCA", motifs, check)


def unused_code():
    """a code whose base no motif uses: codes C+m, C+h and an A code under CG:0 and CCGG:1 alone.  The A code has no row and no summary entry, a site whose only
    entries are the A code's still gives the C codes' rows with those calls in N_other, and a contig listed by the A code's entries alone has its summary rows"""
    contigs = [b"TTCGAACCGGAT", b"AAAA", b"TACGT"]
    t = {K(0, 2, 1, 5): 3,                                          # a C site (CG + at 2) with the A code's entries alone
         K(0, 4, 1, 5): 2, K(0, 10, 1, 5): 4, K(0, 11, -1, 5): 1,    # A sites on both strands: no occurrence there
         K(0, 7, 1, 3): 2, K(0, 7, 1, 0): 1, K(0, 7, 1, 5): 1,       # CG:0 and CCGG:1 share the + site 7
         K(1, 1, 1, 5): 2,                                          # contig 1 is listed by the A code alone
         K(2, 2, 1, 4): 1, K(2, 3, -1, 5): 2}                       # the A code's entries at a - site of CG

    def check(rows, s):
        at = {(r[0], r[1], r[2], r[3], r[4]): r[5:] for r in rows}
        return (not any(r[4] == 2 for r in rows) and not any(x[2] == 2 for x in s)                              # neither a row nor a summary entry of the A code
                and [x[:3] for x in s] == [(c, j, k) for c in range(3) for j in range(2) for k in range(2)]
                and at[(0, 2, 1, 0, 0)] == (0, 0, 3, 0) and at[(0, 2, 1, 0, 1)] == (0, 0, 3, 0)               # its calls are the C codes' N_other
                and at[(0, 7, 1, 0, 0)] == (2, 1, 1, 0) and at[(0, 7, 1, 1, 1)] == (0, 1, 3, 0)
                and at[(2, 3, -1, 0, 0)] == (0, 0, 2, 0) and at[(2, 2, 1, 0, 1)] == (1, 0, 0, 0)
                and not any(r[0] == 0 and r[1] in (4, 10, 11) for r in rows) and not any(r[0] == 1 for r in rows)
                and all(tuple(x[3:]) == (0, 0, 0, 0, 0) for x in s if x[0] == 1)
                and tuple(s[0][3:]) == (4, 2, 1, 3 + 4, 2) and len(rows) == 10)
    return _case("a_code_no_motif_uses", contigs, t, "CCA", [("CG", 0), ("CCGG", 1)], check)


def _lengths():
    rng = np.random.default_rng(72)
    m32 = "GATCNNWWSSRRYYKKMMBDHVACGTACGTAC"
    assert len(m32) == 32
    pick = lambda x: motif_ref.LETTERS[x][int(rng.integers(0, len(motif_ref.LETTERS[x])))]
    hit = "".join(pick(x) for x in m32).encode()
    contigs = [hit, hit[:31], b"TT" + hit + b"T", b"CCCA"]
    t = {K(0, 31, 1, 3): 4, K(0, 0, -1, 0): 1, K(1, 30, 1, 0): 1, K(2, 33, 1, 3): 1, K(2, 33, 1, 0): 1, K(3, 3, 1, 4): 2}
    # A:0 is every A (+) and every T (-); the 32-mer fits contig 0 exactly, not the 31 bases of contig 1, and contig 2 at start 2
    return _case("length_1_and_32", contigs, t, "CA", [(m32, 31), ("A", 0)],
                 lambda rows, s: [_sites(s)[(c, 0, 0)] >= 1 for c in range(3)] == [True, False, True] and _sites(s)[(3, 1, 1)] == 1 and _sites(s)[(0, 1, 1)] == hit.count(b"A") + hit.count(b"T"))


def _letter_sets():
    contigs = [b"TCCAGGTCCTGGTCCGGGTCCNGGT", b"GANTCTGARTCTGAATCTGACTC"]
    t = {K(0, 2, 1, 3): 1, K(0, 8, 1, 3): 1, K(0, 14, 1, 3): 1, K(0, 20, 1, 3): 1, K(0, 4, -1, 3): 2, K(1, 1, 1, 4): 1, K(1, 7, 1, 4): 1, K(1, 13, 1, 4): 1, K(1, 19, 1, 4): 1}
    # CCWGG: CCAGG and CCTGG, not CCGGG, not CCNGG (a reference N fits nothing); GANTC: GAATC and GACTC, not GANTC or GARTC in the reference
    return _case("letter_sets_and_reference_n", contigs, t, "CA", [("CCWGG", 1), ("GANTC", 1)],
                 lambda rows, s: _sites(s) == {(0, 0, 0): 4, (0, 1, 1): 0, (1, 0, 0): 0, (1, 1, 1): 4} and [(r[0], r[1], r[2]) for r in rows] == [(0, 2, 1), (0, 4, -1), (0, 8, 1), (1, 13, 1), (1, 19, 1)])


def _not_palindrome():
    contigs = [b"TTGGTGATTTTTTCACCTT", b"ACGT", b"TTTCACCT"]
    t = {K(0, 6, 1, 3): 3, K(0, 12, -1, 3): 1, K(0, 12, -1, 0): 1, K(0, 12, 1, 0): 9, K(2, 2, -1, 3): 2}      # contig 1 has no entry: not listed
    # GGTGA:4: + at 2..6 (A at 6), - where TCACC lies (T at 12 and at 2 of contig 2); only the - strand of contig 2 has entries
    return _case("own_strand_each_and_a_gap_contig", contigs, t, "A", [("GGTGA", 4)],
                 lambda rows, s: _sites(s) == {(0, 0, 0): 2, (2, 0, 0): 1} and [(r[0], r[1], r[2]) for r in rows] == [(0, 6, 1), (0, 12, -1), (2, 2, -1)])


def _coverage(min_frac, name):
    contigs = [b"TCGTCGTCGTCGTCGTCGT"]
    t = {K(0, 1, 1, 3): 1, K(0, 1, 1, 0): 1,                        # valid 2: below the coverage of 3
         K(0, 4, 1, 3): 1, K(0, 4, 1, 0): 2,                        # valid 3: covered; 1 of 3
         K(0, 7, 1, 1): 9,                                          # fail calls only: valid 0
         K(0, 10, 1, 3): 3, K(0, 10, 1, 0): 7,                      # 3 of 10: at F = 0.3 the product 0.3 * 10 decides
         K(0, 13, 1, 3): 2, K(0, 13, 1, 0): 2,                      # 2 of 4: exactly F = 0.5
         K(0, 16, 1, 3): 2, K(0, 16, 1, 0): 3,                      # 2 of 5: just under 0.5
         K(0, 17, -1, 3): 4, K(0, 17, -1, 1): 1}                    # - strand alone at the last CG
    want = {0.5: 2, 0.3: 4 + (1 if 3.0 >= 0.3 * 10.0 else 0)}[min_frac]
    return _case(name, contigs, t, "C", [("CG", 0)], lambda rows, s: s == [(0, 0, 0, 12, 5, want, 3 + 10 + 4 + 5 + 4, 1 + 3 + 2 + 2 + 4)] and len(rows) == 5, 3, min_frac)


def _combined():
    contigs = [b"TCGTCGTCGTCGTGATCTGATCT", b"TTTT", b"ACGCGT"]
    t = {K(0, 1, 1, 3): 2, K(0, 2, -1, 3): 1, K(0, 2, -1, 0): 1,    # both partners
         K(0, 4, 1, 0): 2,                                          # + alone
         K(0, 8, -1, 3): 3,                                         # - alone: the unit sits at 7
         K(0, 10, 1, 1): 1, K(0, 11, -1, 3): 1,                     # + has fail calls only: it still owns the unit
         K(0, 14, 1, 4): 1, K(0, 15, -1, 4): 2,                     # GATC:1, A at 14, partner T at 15
         K(0, 15, 1, 5): 1,                                         # GATC:2, T at 15 (+), partner A at 14 (-): the partner lies behind
         K(0, 19, -1, 5): 2,                                        # GATC:2 at start 18: - alone at 19, the unit at 20
         K(2, 1, 1, 3): 1, K(2, 4, -1, 3): 1}                       # ACGCGT: units at 1 and 3; the - entry at 4 belongs to the unit at 3

    def check(rows, s):
        at = {(r[0], r[1], r[3], r[4]): r[5:] for r in rows}
        return (all(r[2] == 0 for r in rows) and at[(0, 1, 0, 0)] == (3, 1, 0, 0) and at[(0, 4, 0, 0)] == (0, 2, 0, 0) and at[(0, 7, 0, 0)] == (3, 0, 0, 0)
                and at[(0, 10, 0, 0)] == (1, 0, 0, 1) and at[(0, 14, 1, 1)] == (3, 0, 0, 0) and at[(0, 15, 2, 2)] == (1, 0, 0, 0) and at[(0, 20, 2, 2)] == (2, 0, 0, 0)
                and at[(2, 1, 0, 0)] == (1, 0, 0, 0) and at[(2, 3, 0, 0)] == (1, 0, 0, 0) and _sites(s)[(0, 0, 0)] == 4 and _sites(s)[(2, 0, 0)] == 2
                and [r[:2] for r in rows] == sorted(r[:2] for r in rows))
    return _case("combined_strands", contigs, t, "CAT", [("CG", 0), ("GATC", 1), ("GATC", 2)], check, combine=True)


def cases():
    return [_ends(), _tile_boundary(), _small(), unused_code(), _lengths(), _letter_sets(), _not_palindrome(), _coverage(0.5, "coverage_fail_only_and_f_edges"), _coverage(0.3, "f_times_valid_rounds"),
            _combined()]


def all_in_one(combine):
    """every case's contigs one behind the other with their tables, every class read under the shared codes C+m, C+h and an A code (so class 5, the T code of
    combined_strands, counts as the A code's here), under one set of parameters"""
    contigs, t = [], {}
    for case in cases():
        for key, n in case["table"].items():
            c, pos, strand, cls = mods_ref.unkey(key)
            t[K(c + len(contigs), pos, strand, cls)] = n
        contigs += case["contigs"]
    motifs = [("CG", 0), ("GATC", 1), ("CCWGG", 1), ("GANTC", 1), ("CCGG", 1)] + ([] if combine else [("AA", 0), ("GGTGA", 4), ("A", 0)])
    return dict(name="all_in_one", contigs=contigs, table=t, code_base="CCA", motifs=motifs, min_coverage=2, min_frac=0.5, combine=combine)


def many_units(combine, n=80_000, seed=73):
    """one random contig of 80 000 bases with entries of both C codes and of the A code on both strands at four of five CG and GATC sites: several thousand rows,
    so that the device's ordering of combined units runs at a size beyond one workgroup's"""
    rng = np.random.default_rng(seed)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))
    t = {}
    for q in range(n - 3):
        if seq[q:q + 2] == b"CG":
            for pos, strand in ((q, 1), (q + 1, -1)):
                for cls in (0, 1, 3, 4):
                    if rng.integers(0, 5):
                        t[K(0, pos, strand, cls)] = int(rng.integers(1, 4))
        if seq[q:q + 4] == b"GATC":
            for pos, strand in ((q + 1, 1), (q + 2, -1)):
                if rng.integers(0, 5):
                    t[K(0, pos, strand, 5)] = int(rng.integers(1, 4))
    return dict(name="many_units", contigs=[seq], table=t, code_base="CCA", motifs=[("CG", 0), ("GATC", 1)], min_coverage=2, min_frac=0.5, combine=combine)
