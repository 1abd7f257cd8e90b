"""CPU test of the CLI's --mod-motifs host code (metamaps_amd/csrc/host/motif_out.hpp) through the small driver tests/test_motif_out.cpp, against
tests/motif_ref.py: the option parser (every item shape, every refusal with its message), the reverse-complement test, both writers byte for byte on the rows
and sums of tests/motif_cases.py cut into groups as the CLI cuts them, with and without combined strands, a code whose base no motif uses, and the empty files."""
import os
import subprocess

import pytest

import mods_ref
import motif_cases
import motif_ref

HERE = os.path.dirname(os.path.abspath(__file__))
LIST, CODE_NAME = "C+m,C+h,A+a", ["m", "h", "a"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("motif_out") / "t")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", e,
                    os.path.join(HERE, "test_motif_out.cpp"), "-lz"], check=True, timeout=300)
    return e


def opts(exe, *args):
    p = subprocess.run([exe, "opts"] + list(args), capture_output=True, timeout=60)
    return p.returncode, p.stdout.decode().strip(), p.stderr.decode()


def test_options(exe):
    assert opts(exe) == (0, "0 0.5 0", "")
    assert opts(exe, "mods=" + LIST) == (0, "0 0.5 0", "")
    assert opts(exe, "mods=" + LIST, "mod-motifs=GATC:1,CCWGG:1,CG:0") == (0, "3 0.5 0 | GATC:1 4 1 8 2 | CCWGG:1 2 2 9 4 4 | CG:0 2 4", "")
    assert opts(exe, "mods=" + LIST, "mod-motifs=CG:0,GANTC:1", "mod-motif-min-frac=0.25", "mod-motif-combine-strands")[:2] == (0, "2 0.25 1 | CG:0 2 4 | GANTC:1 4 1 15 8 2")
    every = "ACGTRYSWKMBDHVN"
    assert opts(exe, "mods=" + LIST, "mod-motifs=%s:0,%s:31" % (every, "N" * 31 + "C"))[1].split(" | ")[1] == every + ":0 1 2 4 8 5 10 6 9 12 3 14 13 11 7 15"
    assert opts(exe, "mods=" + LIST, "mod-motifs=" + ",".join("C" * n + ":0" for n in range(1, 9)))[1].startswith("8 ")
    assert opts(exe, "mods=" + LIST, "mod-motifs=CC:0,CC:1,GC:1")[0] == 0                   # the same letters with another offset are another item
    for f in ("0", "1", "1.0", ".5", "0.333"):
        assert opts(exe, "mods=" + LIST, "mod-motifs=CG:0", "mod-motif-min-frac=" + f)[0] == 0, f


def test_every_refusal_carries_the_item(exe):
    m = ["mods=" + LIST]
    syntax = "--mod-motifs takes 1 to 8 comma-separated items MOTIF:OFFSET (1 to 32 IUPAC letters of ACGTRYSWKMBDHVN, ':', the 0-based place of the modified base), not '%s' in '%s'"
    cases = [(["mod-motifs=CG:0"], "--mod-motifs needs --mods"), (["mod-motif-min-frac=0.5"], "--mod-motif-min-frac needs --mods"),
             (["mod-motif-combine-strands"], "--mod-motif-combine-strands needs --mods"), (m + ["mod-motif-min-frac=0.5"], "--mod-motif-min-frac needs --mod-motifs"),
             (m + ["mod-motif-combine-strands"], "--mod-motif-combine-strands needs --mod-motifs")]
    for lst, item in (("", ""), ("CG", "CG"), ("CG:", "CG:"), (":0", ":0"), ("CG:0,", ""), ("cg:0", "cg:0"), ("CXG:0", "CXG:0"), ("CG:x", "CG:x"), ("CG:-1", "CG:-1"), ("CG:0:1", "CG:0:1"),
                      ("CG:100", "CG:100"), ("C" * 33 + ":0", "C" * 33 + ":0"), ("CG:0,C G:0", "C G:0"), (",".join("C" * n + ":0" for n in range(1, 10)), "C" * 9 + ":0")):
        cases.append((m + ["mod-motifs=" + lst], syntax % (item, lst)))
    cases += [(m + ["mod-motifs=CG:0,GATC:4"], "--mod-motifs: the item GATC:4: the offset 4 is not inside the motif's 4 letters"),
              (m + ["mod-motifs=" + "C" * 32 + ":32"], "--mod-motifs: the item " + "C" * 32 + ":32: the offset 32 is not inside the motif's 32 letters"),
              (m + ["mod-motifs=GANTC:2"], "--mod-motifs: the item GANTC:2: the modified base N is not one of A C G T"),
              (m + ["mod-motifs=CCWGG:2"], "--mod-motifs: the item CCWGG:2: the modified base W is not one of A C G T"),
              (m + ["mod-motifs=CG:0,GATC:2"], "--mod-motifs: the item GATC:2: no code of --mods has the base T"),
              (["mods=C+m", "mod-motifs=GATC:1"], "--mod-motifs: the item GATC:1: no code of --mods has the base A"),
              (m + ["mod-motifs=CG:0,GATC:1,CG:0"], "--mod-motifs: the item CG:0 is given twice"),
              (m + ["mod-motifs=CG:0,GGTGA:4,CCAGG:1", "mod-motif-combine-strands"], "--mod-motif-combine-strands: the motif GGTGA is not its own reverse complement"),
              (m + ["mod-motifs=GATC:1,CCAGG:1", "mod-motif-combine-strands"], "--mod-motif-combine-strands: the motif CCAGG is not its own reverse complement")]
    for v in ("", "x", "1.5", "-0.1", "1e-1", "0.5.0", "."):
        cases.append((m + ["mod-motifs=CG:0", "mod-motif-min-frac=" + v], "--mod-motifs: --mod-motif-min-frac takes a decimal from 0 to 1, not '%s'" % v))
    for args, what in cases:
        rc, out, err = opts(exe, *args)
        assert rc == 1 and out == "" and what in err, (args, err)


def test_own_reverse_complement(exe):
    for motif in ("GATC", "CCWGG", "GANTC", "CG", "GGTGA", "CCAGG", "RY", "RR", "N", "A", "W", "S", "ACGT" * 8, "BV", "BB", "KM", "DH", "DD"):
        got = subprocess.run([exe, "rc", motif], capture_output=True, check=True).stdout.strip()
        assert got == (b"1" if motif_ref.own_reverse_complement(motif) else b"0"), motif
    assert motif_ref.own_reverse_complement("GANTC") and not motif_ref.own_reverse_complement("GGTGA") and motif_ref.own_reverse_complement("BV")


def text(exe, args, cname, groups):
    """the two files from (rows, summary) per group"""
    lines = [" ".join(cname)]
    for rows, summary in groups:
        lines += ["R %d %d %d %d %d %d %d" % (mods_ref.key(c, pos, strand if strand else 1, 0), j, k, a, b, o, f) for c, pos, strand, j, k, a, b, o, f in rows]
        lines += ["S " + " ".join(str(x) for x in s) for s in summary] + ["G"]
    p = subprocess.run([exe, "text"] + args, input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    bed, tsv = p.stdout.split(b"==\n")
    return bed, tsv


@pytest.mark.parametrize("combine", [False, True])
def test_both_writers_byte_for_byte(exe, combine):
    w = motif_cases.all_in_one(combine)
    cname = ["contig_%d|x" % c for c in range(len(w["contigs"]))]
    rows, summary = motif_ref.profile(w["contigs"], w["table"], w["code_base"], w["motifs"], w["min_coverage"], w["min_frac"], w["combine"])
    args = ["mods=" + LIST, "mod-motifs=" + ",".join("%s:%d" % m for m in w["motifs"])] + (["mod-motif-combine-strands"] if combine else [])
    want = motif_ref.bedmethyl_text(rows, cname, CODE_NAME, w["motifs"]), motif_ref.tsv_text(summary, cname, CODE_NAME, w["motifs"])
    cut = lambda lo, hi: ([r for r in rows if lo <= r[0] < hi], [s for s in summary if lo <= s[0] < hi])
    n = len(cname)
    assert text(exe, args, cname, [cut(0, n)]) == want
    assert text(exe, args, cname, [cut(c, c + 1) for c in range(n)]) == want
    bed, tsv = want
    assert len(rows) > 100 and all(len(ln.split("\t")) == 18 for ln in bed.decode().splitlines())
    assert {ln.split("\t")[5] for ln in bed.decode().splitlines()} == ({"."} if combine else {"+", "-"})
    lines = tsv.decode().splitlines()
    assert lines[0] == "#contigID\tmotif\toffset\tcode\tsites\tcovered\tmodified\tN_valid_cov\tN_mod\tfraction" and any(ln.endswith("\tNA") for ln in lines)
    stars = [ln.split("\t") for ln in lines if ln.startswith("*\t")]
    assert len(stars) == sum(1 for m, o in w["motifs"] for b in w["code_base"] if b == m[o]) and lines[-len(stars):] == ["\t".join(s) for s in stars]
    for s in stars:                                                # the * rows are the contigs' sums
        assert [int(x) for x in s[4:9]] == [sum(int(ln.split("\t")[4 + k]) for ln in lines[1:] if ln.split("\t")[:4] == [ln.split("\t")[0]] + s[1:4] and not ln.startswith("*")) for k in range(5)]
    assert any(len(s[9].split(".")[1]) == 6 for s in stars if s[9] != "NA")


def test_a_code_no_motif_uses_has_no_line(exe):
    w = motif_cases.unused_code()                                  # codes m, h (C) and a (A) under CG:0 and CCGG:1
    cname = ["contig_%d" % c for c in range(len(w["contigs"]))]
    rows, summary = motif_ref.profile(w["contigs"], w["table"], w["code_base"], w["motifs"], w["min_coverage"], w["min_frac"], w["combine"])
    assert w["check"](rows, summary), "the case misses its point"
    args = ["mods=" + LIST, "mod-motifs=" + ",".join("%s:%d" % m for m in w["motifs"])]
    want = motif_ref.bedmethyl_text(rows, cname, CODE_NAME, w["motifs"]), motif_ref.tsv_text(summary, cname, CODE_NAME, w["motifs"])
    cut = lambda lo, hi: ([r for r in rows if lo <= r[0] < hi], [s for s in summary if lo <= s[0] < hi])
    assert text(exe, args, cname, [cut(0, 3)]) == want
    assert text(exe, args, cname, [cut(c, c + 1) for c in range(3)]) == want
    bed, tsv = (x.decode().splitlines() for x in want)
    assert len(bed) == 10 and {ln.split("\t")[3].split(",")[0] for ln in bed} == {"m", "h"}
    assert len(tsv) == 1 + 3 * 4 + 4 and {ln.split("\t")[3] for ln in tsv[1:]} == {"m", "h"} and [ln.split("\t")[:4] for ln in tsv[-4:]] == [["*", m, str(o), k] for m, o in w["motifs"] for k in "mh"]
    assert bed[0].split("\t")[3:5] + bed[0].split("\t")[11:14] == ["m,CG,0", "3", "0", "0", "3"]          # the A code's three calls at the C site: N_other


def test_the_empty_files(exe):
    assert text(exe, ["mods=" + LIST, "mod-motifs=CG:0"], ["a"], []) == (b"", motif_ref.TSV_HEADER.encode())
