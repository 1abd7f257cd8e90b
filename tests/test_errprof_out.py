"""The text rules of mapDirectly --error-profile (metamaps_amd/csrc/host/errprof_out.hpp: the four writers, their headers and the per-file accumulator) compiled
on their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program (tests/test_errprof_out.cpp), against texts written
down here and against the restatement tests/errprof_ref.py, which the device tests use: the 64+ bin, the `none` row, inf, error rate 1, the * row and the
headers of an empty run.  CPU."""
import os
import subprocess

import pytest

import errprof_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CNAME, CLEN = ["cA", "kraken:taxid|9|cB", "cC"], [7, 2500, 3]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("errprof_out") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_errprof_out.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, counters, listed, rows, total):
    words = list(counters) + [len(listed)] + list(listed) + [v for r in rows + [total] for v in r]
    p = subprocess.run([exe], input=" ".join(str(w) for w in words).encode(), capture_output=True, timeout=120)
    assert p.returncode == 0, (p.stdout + p.stderr).decode(errors="replace")[-3000:]
    parts, name = {}, None
    for ln in p.stdout.decode().splitlines(keepends=True):
        if ln.startswith("== "):
            name = ln[3:-1]; parts[name] = ""
        else:
            parts[name] += ln
    return parts


def world():
    t = errprof_ref.empty_tables()
    for a in range(5):
        for b in range(5):
            t["sub"][a][b] = 1000 * (a == b) + 7 * a + b
    t["indel"][0][1][0] = 40; t["indel"][0][0][0] = 9; t["indel"][0][0][62] = 1; t["indel"][0][1][63] = 2; t["indel"][0][0][63] = 3   # I: 1, 63, 64+
    t["indel"][1][0][1] = 5; t["indel"][1][1][63] = 1                                                                          # D: 2, 64+
    t["qual"][0][0] = 1; t["qual"][1][0] = 2; t["qual"][2][0] = 1           # Q0: rate 0.75
    t["qual"][0][7] = 90; t["qual"][1][7] = 9; t["qual"][2][7] = 1          # Q7: rate 0.1, empirical 10.00
    t["qual"][0][40] = 12345                                                # no error: inf
    t["qual"][1][93] = 3                                                    # nothing but errors: rate 1, empirical 0.00
    t["qual"][0][94] = 10; t["qual"][2][94] = 30                            # none
    listed = [1, 2]
    rows = [[3, 2700, 200, 30, 60, 20, 40, 850_000, 850_000, 900_000, 999_999, 1_000_000], [1, 3, 0, 0, 0, 0, 0, 1_000_000, 1_000_000, 1_000_000, 1_000_000, 1_000_000]]
    total = [4, 2703, 200, 30, 60, 20, 40, 850_000, 850_000, 900_000, 1_000_000, 1_000_000]
    return t, listed, rows, total


def test_the_four_texts(exe):
    t, listed, rows, total = world()
    got = run(exe, errprof_ref.flat(t), listed, rows, total)
    assert got["substitutions"] == ("#truth\tA\tC\tG\tT\tN\nA\t1000\t1\t2\t3\t4\nC\t7\t1008\t9\t10\t11\nG\t14\t15\t1016\t17\t18\nT\t21\t22\t23\t1024\t25\n"
                                    "N\t28\t29\t30\t31\t1032\n")
    assert got["indels"] == "#kind\tlength\thomopolymer\tother\nI\t1\t40\t9\nI\t63\t0\t1\nI\t64+\t2\t3\nD\t2\t0\t5\nD\t64+\t1\t0\n"
    assert got["qualities"] == ("#quality\tmatches\tmismatches\tinserted\terrorRate\tempiricalQ\n0\t1\t2\t1\t0.750000\t1.25\n7\t90\t9\t1\t0.100000\t10.00\n"
                                "40\t12345\t0\t0\t0.000000\tinf\n93\t0\t3\t0\t1.000000\t0.00\nnone\t10\t0\t30\t0.750000\t1.25\n")
    head = ("#contigID\tlength\talignments\treadBases\trefBases\tmatches\tmismatches\tinsertions\tinsertedBases\tdeletions\tdeletedBases\tidentity\tgapCompressedIdentity"
            "\tminIdentity\tq1Identity\tmedianIdentity\tq3Identity\tmaxIdentity\n")
    assert got["contigs"] == (head + "kraken:taxid|9|cB\t2500\t3\t2960\t2940\t2700\t200\t30\t60\t20\t40\t0.900000\t0.915254\t0.850000\t0.850000\t0.900000\t0.999999\t1.000000\n"
                              "cC\t3\t1\t3\t3\t3\t0\t0\t0\t0\t0\t1.000000\t1.000000\t1.000000\t1.000000\t1.000000\t1.000000\t1.000000\n"
                              "*\t2503\t4\t2963\t2943\t2703\t200\t30\t60\t20\t40\t0.900100\t0.915340\t0.850000\t0.850000\t0.900000\t1.000000\t1.000000\n")
    assert got["any quality"] == "1\n"
    assert got["accumulator"] == "twice 5 7 1 2 3 4 5 6 7 8 9 10 11 12\n"
    # the restatement the device tests use writes the same texts
    assert got["substitutions"] == errprof_ref.substitutions_text(t) and got["indels"] == errprof_ref.indels_text(t) and got["qualities"] == errprof_ref.qualities_text(t)
    assert got["contigs"] == errprof_ref.contigs_text(listed, rows, total, CNAME, CLEN)


def test_an_empty_run_writes_the_headers_alone(exe):
    t = errprof_ref.empty_tables()
    got = run(exe, errprof_ref.flat(t), [], [], [0] * 12)
    assert got["substitutions"] == "#truth\tA\tC\tG\tT\tN\n"
    assert got["indels"] == errprof_ref.INDEL_HEADER and got["qualities"] == errprof_ref.QUAL_HEADER and got["contigs"] == errprof_ref.CONTIGS_HEADER
    assert got["any quality"] == "0\n"
    assert got["substitutions"] == errprof_ref.substitutions_text(t) and got["contigs"] == errprof_ref.contigs_text([], [], [0] * 12, CNAME, CLEN)


def test_without_qualities_only_the_none_row(exe):
    t = errprof_ref.empty_tables()
    t["qual"][0][94] = 999; t["qual"][1][94] = 1
    got = run(exe, errprof_ref.flat(t), [], [], [0] * 12)
    assert got["qualities"] == errprof_ref.QUAL_HEADER + "none\t999\t1\t0\t0.001000\t30.00\n" and got["any quality"] == "0\n"
