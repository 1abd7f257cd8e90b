"""The text rules of mapDirectly --consensus (metamaps_amd/csrc/host/consensus_out.hpp: the header and a row of PREFIX.consensus.tsv, the ">contigID" line, the
three thresholds, the groups of contigs) compiled on their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program
(tests/test_consensus_out.cpp).  Every expected value is stated here; the restatement tests/cons_ref.py, which the device tests use, is held to the same
literals.  CPU."""
import os
import subprocess

import pytest

import cons_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = "contigID\tlength\talignments\tcalled\twritten\tconsensusLength\tsnvs\tdeletions\tdeletedBases\tinsertions\tinsertedBases\tdropped\n"
ROW = "kraken:taxid|9|cB\t30000\t200\t28594\t1\t29997\t29\t6\t39\t3\t36\t0\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("consensus_out") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_consensus_out.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.returncode, (p.stdout + p.stderr).decode(errors="replace")[-3000:])
    return p


def test_the_literal_lines(exe):
    assert run(exe, "text").stdout.decode() == HEADER + ROW + ">kraken:taxid|9|cB\n"
    stats = dict(zip(cons_ref.STATS, (200, 28594, 1, 29997, 29, 6, 39, 3, 36, 0)))
    res = {1: (stats, "ACGT" * 16, {})}
    assert cons_ref.TSV_HEADER == HEADER and cons_ref.tsv_text(res, ["cA", "kraken:taxid|9|cB"], [7, 30000]).decode() == HEADER + ROW
    assert cons_ref.fasta_text(res, ["cA", "kraken:taxid|9|cB"]).decode() == ">kraken:taxid|9|cB\n" + "ACGT" * 15 + "\nACGT\n"


def test_thresholds(exe):
    assert run(exe, "opts").stdout.split() == [b"0", b"3", b"0.5", b"0"]
    assert run(exe, "opts", "consensus", "1").stdout.split() == [b"1", b"3", b"0.5", b"0"]
    assert run(exe, "opts", "consensus", "1", "consensus-min-depth", "1", "consensus-min-frac", "1", "consensus-min-called", "1").stdout.split() == [b"1", b"1", b"1", b"1"]
    assert run(exe, "opts", "consensus", "1", "consensus-min-depth", "250", "consensus-min-frac", ".75", "consensus-min-called", "0.25").stdout.split() == [b"1", b"250", b"0.75", b"0.25"]
    assert run(exe, "opts", "vcf", "1", "vcf-min-frac", "0.1", "consensus", "1").stdout.split() == [b"1", b"3", b"0.5", b"0"]   # the VCF's are not ours
    for bad in (["consensus-min-depth", "0"], ["consensus-min-depth", "-1"], ["consensus-min-depth", "2.5"], ["consensus-min-depth", ""], ["consensus-min-depth", "1e3"],
                ["consensus-min-frac", "0.49"], ["consensus-min-frac", "1.5"], ["consensus-min-frac", "."], ["consensus-min-frac", "0.5.2"], ["consensus-min-frac", "half"],
                ["consensus-min-called", "1.01"], ["consensus-min-called", "-0.1"], ["consensus-min-called", ""], ["consensus-min-called", "all"]):
        p = run(exe, "opts", "consensus", "1", *bad, rc=1)
        assert b"--consensus" in p.stderr and bad[0].encode() in p.stderr and p.stdout == b"", bad
        p = run(exe, "opts", *bad, rc=1)                            # without --consensus: refused whatever the value
        assert b"needs --consensus" in p.stderr, bad
    assert b"needs --consensus" in run(exe, "opts", "vcf", "1", "consensus-min-frac", "0.5", rc=1).stderr


def groups(exe, max_bases, clen, contigs):
    return [tuple(int(x) for x in ln.split()) for ln in run(exe, "groups", max_bases, *clen, ":", *contigs).stdout.decode().splitlines()]


def test_groups(exe):
    clen = [100, 50, 70, 30, 200, 10]
    iv = [4, 0, 2, 2, 0, 3, 4]                                      # contigs 1 and 5 have no interval
    assert groups(exe, 1, clen, iv) == [(0, 1), (2, 3), (3, 4), (4, 5)]                # a bound of one base: every contig with an interval alone
    assert groups(exe, 100, clen, iv) == [(0, 1), (2, 4), (4, 5)]                      # one contig's length: 70 + 30 fit, 100 + 50 + 70 do not
    assert groups(exe, 220, clen, iv) == [(0, 3), (3, 4), (4, 5)]                      # the contig without an interval in between counts: 100 + 50 + 70
    assert groups(exe, 249, clen, iv) == [(0, 3), (3, 5)]
    assert groups(exe, 250, clen, iv) == [(0, 4), (4, 5)]
    assert groups(exe, sum(clen), clen, iv) == [(0, 5)]                                 # everything: the trailing contig without an interval stays out
    assert groups(exe, 1 << 40, clen, iv) == [(0, 5)]
    assert groups(exe, 100, clen, []) == []
    assert groups(exe, 5, clen, [5, 5, 5]) == [(5, 6)]
    for bound in (1, 60, 100, 230, 1000):                           # every contig with an interval lies in exactly one group, which starts and ends at one
        got = groups(exe, bound, clen, iv)
        assert sorted(c for lo, hi in got for c in range(lo, hi) if c in iv) == sorted(set(iv))
        assert all(lo in iv and hi - 1 in iv and (hi - lo == 1 or sum(clen[lo:hi]) <= bound) for lo, hi in got)
