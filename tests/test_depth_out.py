"""The text rules of mapDirectly --depth (metamaps_amd/csrc/host/depth_out.hpp: the lines of PREFIX.depth.bedgraph, .depth.windows and .depth.contigs, the header,
the window and the thresholds) compiled on their own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone program
(tests/test_depth_out.cpp).  Integer columns are compared byte for byte; the %.3f / %.6f columns as numbers within 1e-3 / 1e-6, their print resolution (the C
library's exp and Python's need not agree in the last bit).  The restatement tests/depth_ref.py, which the device tests use, is held to the same texts.  CPU."""
import os
import subprocess

import pytest

import depth_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CNAME, CLEN = ["cA", "kraken:taxid|9|cB", "cC"], [7, 2500, 3]
FLOATS = {"windows": {5: 1e-3}, "contigs": {5: 1e-3, 8: 1e-6, 9: 1e-6}}   # column: resolution


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("depth_out") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_depth_out.cpp"), "-lpthread"], check=True, timeout=600)
    return p


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.returncode, (p.stdout + p.stderr).decode(errors="replace")[-3000:])
    return p


def same_text(got, want, floats):
    """integer and name columns byte for byte, the columns of `floats` as numbers within their resolution and in their printed form"""
    g, w = got.splitlines(keepends=True), want.splitlines(keepends=True)
    assert len(g) == len(w), (got, want)
    for a, b in zip(g, w):
        assert a.endswith("\n") and b.endswith("\n")
        ca, cb = a[:-1].split("\t"), b[:-1].split("\t")
        assert len(ca) == len(cb), (a, b)
        for k, (x, y) in enumerate(zip(ca, cb)):
            if k in floats and not a.startswith("#"):
                assert abs(float(x) - float(y)) <= floats[k] * 1.0000001 and len(x.split(".")[1]) == len(y.split(".")[1]), (a, b)
            else:
                assert x == y, (a, b)


def profile(thresholds):
    n = len(thresholds)
    return dict(runs=[(1, 0, 1000, 1), (1, 1000, 1700, 4), (2, 0, 3, 70000)], contig=[1, 2], win_off=[0, 3, 4],
                stats=[[3, 1700, 4100, 1, 4] + [1700 - 100 * k for k in range(n)], [70000, 3, 210000, 70000, 70000] + [3] * n],
                win_sum=[1000, 2800, 0, 210000], win_covered=[1000, 700, 0, 3])


def sections(out):
    parts = out.decode().split("== ")
    assert parts[0] == ""
    return {p.split("\n", 1)[0]: p.split("\n", 1)[1] for p in parts[1:]}


@pytest.mark.parametrize("thresholds", [(1, 5, 10, 30), (3,), (1, 2, 3, 4, 5, 6, 7, 800000)])
def test_the_three_texts(exe, thresholds):
    args = ["depth", "1"] + ([] if thresholds == (1, 5, 10, 30) else ["depth-thresholds", ",".join(map(str, thresholds))])
    got = sections(run(exe, "text", *args).stdout)
    res = profile(thresholds)
    assert got["bedgraph"] == depth_ref.bedgraph_text(res, CNAME) == "kraken:taxid|9|cB\t0\t1000\t1\nkraken:taxid|9|cB\t1000\t1700\t4\ncC\t0\t3\t70000\n"
    same_text(got["windows"], depth_ref.windows_text(res, CNAME, CLEN, 1000), FLOATS["windows"])
    same_text(got["contigs"], depth_ref.contigs_text(res, CNAME, CLEN, thresholds), FLOATS["contigs"])
    assert got["empty"] == depth_ref.contigs_header(thresholds)    # an empty run: two empty files and the header alone
    if thresholds == (1, 5, 10, 30):                                # the literal lines
        assert got["windows"] == ("kraken:taxid|9|cB\t0\t1000\t1000\t1000\t1.000\nkraken:taxid|9|cB\t1000\t2000\t2800\t700\t2.800\nkraken:taxid|9|cB\t2000\t2500\t0\t0\t0.000\n"
                                  "cC\t0\t3\t210000\t3\t70000.000\n")
        lines = got["contigs"].splitlines()
        assert lines[0] == "#contigID\tlength\talignments\tcovered\tsumDepth\tmeanDepth\tmedianDepth\tmaxDepth\tbreadth\texpectedBreadth\tge1\tge5\tge10\tge30"
        assert lines[1].split("\t")[:9] == ["kraken:taxid|9|cB", "2500", "3", "1700", "4100", "1.640", "1", "4", "0.680000"] and lines[1].split("\t")[10:] == ["1700", "1600", "1500", "1400"]
        assert abs(float(lines[1].split("\t")[9]) - 0.806020) <= 1e-6   # 1 - exp(-1.64)
        assert lines[2] == "cC\t3\t70000\t3\t210000\t70000.000\t70000\t70000\t1.000000\t1.000000\t3\t3\t3\t3"


def test_options(exe):
    assert run(exe, "opts").stdout.split() == [b"0", b"1000", b"1,5,10,30"]
    assert run(exe, "opts", "depth", "1").stdout.split() == [b"1", b"1000", b"1,5,10,30"]
    assert run(exe, "opts", "depth", "1", "depth-window", "1", "depth-thresholds", "7").stdout.split() == [b"1", b"1", b"7"]
    assert run(exe, "opts", "depth", "1", "depth-window", "536870911", "depth-thresholds", "1,2,3,4,5,6,7,8").stdout.split() == [b"1", b"536870911", b"1,2,3,4,5,6,7,8"]
    for bad in (["depth-window", "0"], ["depth-window", "-1"], ["depth-window", "2.5"], ["depth-window", ""], ["depth-window", "1e3"], ["depth-window", "1000000000000"],
                ["depth-thresholds", ""], ["depth-thresholds", "0"], ["depth-thresholds", "0,5"], ["depth-thresholds", "5,5"], ["depth-thresholds", "10,5"], ["depth-thresholds", "1,,5"],
                ["depth-thresholds", "1,5,"], ["depth-thresholds", ",1"], ["depth-thresholds", "1;5"], ["depth-thresholds", "1,2,3,4,5,6,7,8,9"], ["depth-thresholds", "1,x"]):
        p = run(exe, "opts", "depth", "1", *bad, rc=1)
        assert b"--depth" in p.stderr and bad[0].encode() in p.stderr and p.stdout == b"", bad
        p = run(exe, "opts", *bad, rc=1)                            # without --depth: refused whatever the value
        assert b"needs --depth" in p.stderr, bad
    assert b"needs --depth" in run(exe, "opts", "pileup", "1", "depth-window", "100", rc=1).stderr
