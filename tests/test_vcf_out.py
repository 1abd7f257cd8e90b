"""The text rules of mapDirectly --vcf (metamaps_amd/csrc/host/vcf_out.hpp: the header and the five line shapes of PREFIX.vcf, the two thresholds) compiled on
their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program (tests/test_vcf_out.cpp).  Every expected value is
stated here; the restatement tests/vcf_ref.py, which the device tests use, is held to the same literals.  CPU."""
import os
import subprocess

import pytest

import vcf_ref

HERE = os.path.dirname(os.path.abspath(__file__))

HEADER = ('##fileformat=VCFv4.2\n##source=metamaps mapDirectly --vcf\n##contig=<ID=cA,length=100>\n##contig=<ID=kraken:taxid|9|cB,length=4000000>\n##contig=<ID=cC,length=7>\n'
          '##INFO=<ID=DP,Number=1,Type=Integer,Description="Primary alignments that span the position">\n'
          '##INFO=<ID=AO,Number=1,Type=Integer,Description="Primary alignments that carry the allele">\n'
          '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of a symbolic allele">\n'
          '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Length of a symbolic allele, negative for a deletion">\n'
          '##INFO=<ID=END,Number=1,Type=Integer,Description="Last reference position of a symbolic allele">\n'
          '##ALT=<ID=INS,Description="Insertion of more than 24 bases">\n##ALT=<ID=DEL,Description="Deletion of more than 24 bases">\n'
          '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
LINES = ["cA\t1\t.\tA\tC\t.\t.\tDP=3;AO=3",                                            # an SNV
         "cA\t10\t.\tTNNA\tT\t.\t.\tDP=40;AO=12",                                      # a deletion of 3: r and N of the reference print as N
         "cA\t10\t.\tN\tNGAT\t.\t.\tDP=40;AO=4",                                       # an insertion of GAT behind a lower-case n
         "cA\t41\t.\tG\t<DEL>\t.\t.\tDP=50;AO=5;SVTYPE=DEL;SVLEN=-25;END=66",
         "kraken:taxid|9|cB\t4000000\t.\tC\t<INS>\t.\t.\tDP=4000000001;AO=4000000000;SVTYPE=INS;SVLEN=30;END=4000000",
         "kraken:taxid|9|cB\t4000000\t.\tN\tT\t.\t.\tDP=9;AO=1",
         "cC\t3\t.\tC" + "A" * 24 + "\tC\t.\t.\tDP=2;AO=2",                             # 24 bases are still spelt out
         "cC\t7\t.\tG\tG" + "TGCA" * 6 + "\t.\t.\tDP=7;AO=7"]
CNAME = ["cA", "kraken:taxid|9|cB", "cC"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vcf_out") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_vcf_out.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.returncode, (p.stdout + p.stderr).decode(errors="replace")[-3000:])
    return p


def test_the_header(exe):
    assert run(exe, "header").stdout.decode() == HEADER
    assert vcf_ref.header_text(CNAME, [100, 4000000, 7]).decode() == HEADER


def test_each_of_the_five_line_shapes(exe):
    assert run(exe, "lines").stdout.decode().splitlines() == LINES


def test_the_restatement_prints_the_same_lines():
    K, w = vcf_ref.key, lambda s: s.encode().ljust(25, b"\0")
    entries = [(*K((0, 0, "S", "C")), 3, 3, w("ACGT")), (*K((0, 9, "D", 3)), 12, 40, w("TRNA")), (*K((0, 9, "I", "GAT")), 4, 40, w("NCGT")),
               (*K((0, 40, "D", 25)), 5, 50, w("GACGTACGTACGTACGTACGTACGT")), (*K((1, 3999999, "I", "A" * 30)), 4000000000, 4000000001, w("C")),
               (*K((1, 3999999, "S", "T")), 1, 9, w("Y")), (*K((2, 2, "D", 24)), 2, 2, w("C" + "A" * 24)), (*K((2, 6, "I", "TGCA" * 6)), 7, 7, w("G"))]
    assert [vcf_ref.line(e, CNAME) for e in entries] == [ln + "\n" for ln in LINES]


def test_thresholds(exe):
    assert run(exe, "opts").stdout.split() == [b"0", b"3", b"0.20000000000000001"]
    assert run(exe, "opts", "vcf", "1").stdout.split() == [b"1", b"3", b"0.20000000000000001"]
    assert run(exe, "opts", "vcf", "1", "vcf-min-count", "1", "vcf-min-frac", "0").stdout.split() == [b"1", b"1", b"0"]
    assert run(exe, "opts", "vcf", "1", "vcf-min-count", "250", "vcf-min-frac", "1").stdout.split() == [b"1", b"250", b"1"]
    assert run(exe, "opts", "vcf", "1", "vcf-min-frac", ".5").stdout.split() == [b"1", b"3", b"0.5"]
    assert run(exe, "opts", "pileup", "1", "pileup-min-count", "7", "vcf", "1").stdout.split() == [b"1", b"3", b"0.20000000000000001"]   # the pileup's are not ours
    for bad in (["vcf-min-count", "0"], ["vcf-min-count", "-1"], ["vcf-min-count", "2.5"], ["vcf-min-count", ""], ["vcf-min-count", "1e3"],
                ["vcf-min-frac", "1.5"], ["vcf-min-frac", "-0.1"], ["vcf-min-frac", "."], ["vcf-min-frac", "0.1.2"], ["vcf-min-frac", "half"]):
        p = run(exe, "opts", "vcf", "1", *bad, rc=1)
        assert b"--vcf" in p.stderr and bad[0].encode() in p.stderr and p.stdout == b"", bad
        p = run(exe, "opts", *bad, rc=1)                            # without --vcf: refused whatever the value
        assert b"needs --vcf" in p.stderr, bad
    assert b"needs --vcf" in run(exe, "opts", "vcf-min-count", "2", rc=1).stderr
    assert b"needs --vcf" in run(exe, "opts", "pileup", "1", "vcf-min-frac", "0.5", rc=1).stderr
