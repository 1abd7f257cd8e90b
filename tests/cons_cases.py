"""Tables for the tests of mapDirectly --consensus (metamaps_amd/csrc/mm_cons_core.hpp on the host, mm_consensus on the device): the smallest shapes at which
the select rule, the per-position output and the line wrap can go wrong.  A world is a dict: contigs (byte strings), t ({(w0, w1): count}, vcf_ref.py's
table), iv ((contig, first, last)), D, F, C and width; in the built world every case is a contig of its own, named in CASES."""
import numpy as np

import edit_cases
import vcf_ref

K = vcf_ref.key
S = lambda c, p, alt: K((c, p, "S", alt))
DL = lambda c, a, n: K((c, a, "D", n))
IN = lambda c, a, s: K((c, a, "I", s))


def other(b, k=1):
    """the k-th letter of ACGT behind the contig's byte"""
    return "ACGT"[("ACGT".index(chr(b).upper()) + k) % 4]


CASES = ("ends", "del_to_end", "tie", "d123", "on_removed", "two_ins", "ins_24_25", "big", "depth", "ref_bytes", "len59", "len60", "len61", "len120", "straddle",
         "no_intervals", "nothing_called")


def built_world():
    rng = np.random.default_rng(301)
    length = dict.fromkeys(CASES, 100)
    length.update(big=66_000, len59=59, len60=60, len61=61, len120=120)
    contigs = [bytearray(edit_cases.dna(rng, length[name])) for name in CASES]
    c = {name: k for k, name in enumerate(CASES)}
    t, iv = {}, []

    def cover(name, depth=4, first=0, last=None):
        iv.extend([(c[name], first, length[name] - 1 if last is None else last)] * depth)
    ref = lambda name, p: contigs[c[name]][p]
    # an SNV and an insertion at position 0 and at the last base
    cover("ends")
    t[S(c["ends"], 0, other(ref("ends", 0)))] = 4; t[S(c["ends"], 99, other(ref("ends", 99)))] = 3
    t[IN(c["ends"], 0, "GT")] = 4; t[IN(c["ends"], 99, "A")] = 2
    cover("del_to_end")                                             # the footprint [96, 99] ends at the last base
    t[DL(c["del_to_end"], 95, 4)] = 4
    cover("tie")                                                    # 2 / 2 at depth 4 and F = 0.5: the lower code wins
    contigs[c["tie"]][50] = ord("A")
    t[S(c["tie"], 50, "C")] = 2; t[S(c["tie"], 50, "T")] = 2
    cover("d123")                                                   # D1 [10, 20], D2 [15, 25], D3 [22, 30]: only D1; the abutting pair [51, 55] and [56, 58]: both
    t[DL(c["d123"], 9, 11)] = 4; t[DL(c["d123"], 14, 11)] = 3; t[DL(c["d123"], 21, 9)] = 3
    t[DL(c["d123"], 50, 5)] = 3; t[DL(c["d123"], 55, 3)] = 3
    cover("on_removed")                                             # deletion [21, 30]; an SNV and an INS at 25 (removed); an INS and an SNV on its anchor 20; both at 60
    k = c["on_removed"]
    t[DL(k, 20, 10)] = 4; t[S(k, 25, other(ref("on_removed", 25)))] = 4; t[IN(k, 25, "C")] = 4; t[IN(k, 20, "TTG")] = 3; t[S(k, 20, other(ref("on_removed", 20)))] = 2
    t[S(k, 60, other(ref("on_removed", 60), 2))] = 4; t[IN(k, 60, "ACGT")] = 4
    cover("two_ins")                                                # two candidate insertions at one anchor (AO <= DP does not hold inside repeats)
    t[IN(c["two_ins"], 40, "CG")] = 3; t[IN(c["two_ins"], 40, "A")] = 3
    cover("ins_24_25")
    t[IN(c["ins_24_25"], 30, "ACGTTGCA" * 3)] = 4; t[IN(c["ins_24_25"], 40, "A" * 25)] = 4
    # a deletion of 65 535; deletions and insertions of 64 and 65 (a lane's own run, and the wavefront's), a long symbolic insertion
    cover("big", 3)
    k = c["big"]
    t[DL(k, 50, 65535)] = 3; t[DL(k, 65600, 64)] = 3; t[DL(k, 65700, 65)] = 3
    t[IN(k, 65800, "G" * 64)] = 3; t[IN(k, 65810, "G" * 65)] = 3; t[IN(k, 65820, "G" * 200)] = 2
    # depth exactly D on [10, 50] and D - 1 on [51, 60]; an interval's last base 80 and the one behind it
    k = c["depth"]
    iv.extend([(k, 10, 60)] * 2 + [(k, 10, 50)] + [(k, 70, 80)] * 3)
    for p in (50, 51, 80, 81):
        t[S(k, p, other(ref("depth", p)))] = 3 if p != 51 else 2
    cover("ref_bytes")                                              # bytes that are no base, and a lower-case one
    contigs[c["ref_bytes"]][20:24] = b"NRna"
    for name in ("len59", "len60", "len61", "len120"):
        cover(name)
    cover("straddle")                                               # columns 58 .. 62 of a line of 60
    t[IN(c["straddle"], 57, "ACGTA")] = 4
    t[S(c["no_intervals"], 10, other(ref("no_intervals", 10)))] = 5  # rows without an interval: depth 0
    cover("nothing_called", 2)
    t[S(c["nothing_called"], 10, other(ref("nothing_called", 10)))] = 2
    return dict(contigs=[bytes(x) for x in contigs], t=t, iv=iv, D=3, F=0.5, C=0.0, width=60)


def called_world():
    """C = 0.5: 50 called positions of 100 are exactly ceil(C * len), 50 of 101 lie below"""
    rng = np.random.default_rng(302)
    contigs = [edit_cases.dna(rng, 100), edit_cases.dna(rng, 101), edit_cases.dna(rng, 100)]
    return dict(contigs=contigs, t={S(1, 5, other(contigs[1][5])): 1}, iv=[(0, 0, 49), (1, 0, 49), (2, 0, 48)], D=1, F=0.5, C=0.5, width=60)


COMBOS = ((3, 0.5, 0.0, 60), (1, 0.5, 0.3, 7), (2, 0.6, 0.9, 1), (2, 1.0, 0.0, 61))   # (D, F, C, width) of the random tables


def random_worlds(n=200, seed=303):
    """tables over low-complexity contigs whose rows crowd into a few zones, so that deletions overlap and SNVs and insertions fall on removed positions"""
    rng = np.random.default_rng(seed)
    out = []
    for w in range(n):
        D, F, C, width = COMBOS[w % len(COMBOS)]
        contigs, t, iv = [], {}, []
        for c in range(int(rng.integers(1, 4))):
            m = int(rng.integers(30, 260))
            s = bytearray()
            while len(s) < m:
                kind = int(rng.integers(0, 4))
                s += (edit_cases.dna(rng, int(rng.integers(5, 40))) if kind == 0 else bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(3, 30)) if kind == 1
                      else edit_cases.dna(rng, int(rng.integers(2, 5))) * int(rng.integers(2, 12)) if kind == 2 else bytes([b"NRn"[int(rng.integers(0, 3))]]))
            contigs.append(bytes(s[:m]))
            if rng.random() < 0.1:
                continue                                            # a contig without an interval
            for _ in range(int(rng.integers(1, 14))):
                a = int(rng.integers(0, m)) if rng.random() < 0.5 else 0
                iv.append((c, a, int(rng.integers(a, m)) if rng.random() < 0.7 else m - 1))
            depth = [sum(1 for cc, a, b in iv if cc == c and a <= p <= b) for p in range(m)]
            zones = [int(rng.integers(0, m)) for _ in range(3)]
            for _ in range(int(rng.integers(0, 40))):
                p = min(m - 1, max(0, zones[int(rng.integers(0, 3))] + int(rng.integers(-6, 7)))) if rng.random() < 0.8 else int(rng.integers(0, m))
                count = max(1, int(rng.integers(depth[p] // 2, depth[p] + 2)))
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    t[S(c, p, "ACGT"[int(rng.integers(0, 4))])] = count
                elif kind == 1 and p + 1 < m - 1:
                    t[DL(c, p, int(rng.integers(1, min(m - 1 - p, 70 if rng.random() < 0.1 else 9))))] = count
                elif kind == 2:
                    size = int(rng.integers(1, 6)) if rng.random() < 0.8 else int(rng.integers(20, 80))
                    t[IN(c, p, "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=size)))] = count
        out.append(dict(contigs=contigs, t=t, iv=iv, D=D, F=F, C=C, width=width))
    return out


def joined(worlds):
    """worlds with the same thresholds as one: the contigs behind one another"""
    first = worlds[0]
    out = dict(contigs=[], t={}, iv=[], D=first["D"], F=first["F"], C=first["C"], width=first["width"])
    for w in worlds:
        assert (w["D"], w["F"], w["C"], w["width"]) == (out["D"], out["F"], out["C"], out["width"])
        base = len(out["contigs"])
        out["contigs"] += w["contigs"]
        out["t"].update({(k[0] + (base << 35), k[1]): n for k, n in w["t"].items()})
        out["iv"] += [(c + base, a, b) for c, a, b in w["iv"]]
    return out


def refused_worlds():
    """(why, world): what the definition does not take"""
    rng = np.random.default_rng(304)
    contigs = [edit_cases.dna(rng, 100), edit_cases.dna(rng, 30)]
    good = dict(contigs=contigs, t={S(0, 5, "A"): 3, DL(0, 5, 3): 3}, iv=[(0, 0, 99)] * 3, D=3, F=0.5, C=0.0, width=60)
    out = [("D < 1", dict(good, D=0)), ("F < 0.5", dict(good, F=0.49)), ("F > 1", dict(good, F=1.01)), ("C < 0", dict(good, C=-0.1)), ("C > 1", dict(good, C=1.5)),
           ("width < 1", dict(good, width=0))]
    out.append(("not ascending", dict(good, order=[DL(0, 5, 3), S(0, 5, "A")])))
    out.append(("not unique", dict(good, order=[S(0, 5, "A"), S(0, 5, "A")])))
    for why, key in (("position past the contig", S(0, 100, "A")), ("contig past the reference", S(2, 0, "A")), ("code 7", (S(0, 5, "A")[0] | 7, 0)), ("code 4", (S(0, 5, "A")[0] & ~7 | 4, 0)),
                     ("an SNV with a second word", (S(0, 5, "A")[0], 1)), ("a deletion past the end", DL(0, 5, 95)), ("a deletion of 0", (DL(0, 5, 1)[0], 0)),
                     ("a deletion of 2^16", (DL(0, 5, 1)[0], 1 << 16)), ("an insertion of 0", (IN(0, 5, "A")[0], 0)), ("bases beyond the length", (IN(0, 5, "A")[0], 1 << 48 | 4)),
                     ("bases of a symbolic insertion", (IN(0, 5, "A")[0], 25 << 48 | 1))):
        out.append((why, dict(good, t={key: 3})))
    for why, x in (("an interval past its contig", (0, 5, 100)), ("an empty interval", (0, 6, 5)), ("an interval of no contig", (2, 0, 5)), ("a negative first", (0, -1, 5))):
        out.append((why, dict(good, iv=[x])))
    return good, out
