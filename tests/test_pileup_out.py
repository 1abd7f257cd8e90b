"""The text rules of mapDirectly --pileup (metamaps_amd/csrc/host/pileup_out.hpp: the lines of PREFIX.pileup and PREFIX.pileup.contigs, which records
contribute, the two thresholds) compiled on their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program
(tests/test_pileup_out.cpp).  Every expected value is stated here.  CPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pileup_out") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_pileup_out.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.returncode, (p.stdout + p.stderr).decode(errors="replace")[-3000:])
    return p


def test_the_lines_of_both_files(exe):
    """every alt letter's column, positions 0 and 3 999 999, counts beyond 2^31; a contig without an alignment has no line in .contigs"""
    sites, contigs = run(exe, "text").stdout.decode().split("--\n")
    assert sites == ("cA\t0\tA\tC\t3\t3\ncA\t99\tN\t-\t12\t40\nkraken:taxid|9|cB\t3999999\tg\t+\t4000000000\t4000000001\n"
                     "kraken:taxid|9|cB\t3999999\tT\tN\t1\t9\ncC\t3\tC\tT\t2\t2\n")
    assert contigs == "cA\t100\t6\t51\t65\ncC\t7\t1\t7\t5000000000\n"


def test_only_the_primary_aligned_record_contributes(exe):
    got = run(exe, "use", "0,5", "256,5", "16,0", "272,3", "0,-1", "16,-1").stdout.split()
    assert got == [b"1", b"0", b"1", b"0", b"0", b"0"]


def test_thresholds(exe):
    assert run(exe, "opts").stdout.split() == [b"0", b"3", b"0.20000000000000001"]
    assert run(exe, "opts", "pileup", "1").stdout.split() == [b"1", b"3", b"0.20000000000000001"]
    assert run(exe, "opts", "pileup", "1", "pileup-min-count", "1", "pileup-min-frac", "0").stdout.split() == [b"1", b"1", b"0"]
    assert run(exe, "opts", "pileup", "1", "pileup-min-count", "250", "pileup-min-frac", "1").stdout.split() == [b"1", b"250", b"1"]
    assert run(exe, "opts", "pileup", "1", "pileup-min-frac", ".5").stdout.split() == [b"1", b"3", b"0.5"]
    for bad in (["pileup-min-count", "0"], ["pileup-min-count", "-1"], ["pileup-min-count", "2.5"], ["pileup-min-count", ""], ["pileup-min-count", "1e3"],
                ["pileup-min-frac", "1.5"], ["pileup-min-frac", "-0.1"], ["pileup-min-frac", "."], ["pileup-min-frac", "0.1.2"], ["pileup-min-frac", "half"]):
        p = run(exe, "opts", "pileup", "1", *bad, rc=1)
        assert b"--pileup" in p.stderr and bad[0].encode() in p.stderr and p.stdout == b"", bad
        p = run(exe, "opts", *bad, rc=1)                            # without --pileup: refused whatever the value
        assert b"needs --pileup" in p.stderr, bad
    assert b"needs --pileup" in run(exe, "opts", "pileup-min-count", "2", rc=1).stderr
