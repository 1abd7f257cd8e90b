"""The word-level functions of homopolymer compression (metamaps_amd/csrc/mm_hpc_core.hpp: keep mask, field extraction, select, the
raw / rawlast look-up) built with g++, plain and under ASan/UBSan, against itertools.groupby.  CPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def hpc(s):
    """(compressed text, raw position of the first base of every run, of the last base of every run)"""
    out, first, last, at = [], [], [], 0
    for ch, grp in itertools.groupby(s):
        n = len(list(grp))
        out.append(ch); first.append(at); last.append(at + n - 1)
        at += n
    return "".join(out), first, last


def raw_maps(s, beyond):
    """raw(p), rawlast(p) for p in 0 .. clen + beyond - 1 by the definition: beyond the end both are rawlen + (p - clen)"""
    c, first, last = hpc(s)
    ext = [len(s) + j for j in range(beyond)]
    return c, first + ext, last + ext


def cases():
    rng = np.random.default_rng(7)
    rnd = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    alt = lambda n: "".join("AC"[j & 1] for j in range(n))
    nodup = lambda n: "".join("ACGT"[(j * 3 + j // 4) & 3] if j % 4 else "ACGT"[(j // 4 + 1) & 3] for j in range(n))
    S = [rnd(n) for n in (0, 1, 15, 16, 17, 31, 32, 33)]
    S += ["A" * n for n in (1, 15, 16, 17, 33)] + ["T" * 40, "G" * 16, "C" * 64]
    S += [alt(n) for n in (15, 16, 17, 32, 33, 70)]
    S += ["AC" * 5 + "G" * k + "T" + "ACGT" * 5 for k in (5, 6, 7)]       # a run that ends at base 15, 16 and 17 of a word (1-based)
    S += ["ACG" + "T" * 45 + "GCA", "T" * 48 + "A", "CA" + "G" * 30]     # runs spanning three words
    S += ["", "", rnd(100), "", "A" * 700 + "C" + "G" * 900 + rnd(50), rnd(5000)]
    S += ["".join(ch * int(rng.integers(1, 4)) for ch in rnd(900))]      # more than 512 kept bases: the second select sample is used
    S += ["ACGT" * 8 + "T", "T" * 16, "T" + "ACGT" * 4]                  # neighbours that end and begin with the same base must not merge
    return S


def build(tmp, flags):
    p = str(tmp / ("t" + str(len(flags))))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", p, os.path.join(HERE, "test_hpc_core.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpc")
    return {"plain": build(d, []), "san": build(d, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


@pytest.mark.parametrize("kind", ["plain", "san"])
def test_header_matches_groupby(exes, kind):
    S = cases()
    p = subprocess.run([exes[kind]], input=("\n".join(S) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")
    assert len(lines) >= 2 * len(S)
    for i, s in enumerate(S):
        c, first, last = raw_maps(s, 3)
        assert lines[2 * i] == c, (i, s[:60])
        got = [tuple(int(x) for x in t.split(":")) for t in lines[2 * i + 1].split()]
        assert [g[0] for g in got] == first, (i, s[:60])
        assert [g[1] for g in got] == last, (i, s[:60])


def test_definition_examples():
    assert hpc("NNNN")[0] == "N" and hpc("aAaA".upper())[0] == "A" and hpc("NNRRNN")[0] == "NRN" and hpc("")[0] == ""
    c, first, last = raw_maps("AAACCG", 2)
    assert (c, first, last) == ("ACG", [0, 3, 5, 6, 7], [2, 4, 5, 6, 7])
