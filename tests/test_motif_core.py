"""The definition of methylation per motif (metamaps_amd/csrc/mm_motif_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the
address and undefined-behaviour sanitizers — against the plain restatement tests/motif_ref.py on the cases of tests/motif_cases.py, each of which is first
asserted to exercise what it is named for.  CPU."""
import os
import subprocess

import pytest

import mods_ref
import motif_cases
import motif_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = motif_cases.cases()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("motif_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_motif_core.cpp")], check=True, timeout=300)
    return p


def world_text(w):
    keys = sorted(w["table"])
    head = f"{len(w['contigs'])} {len(keys)} {w['code_base']} {len(w['motifs'])} {w['min_coverage']} {float(w['min_frac']).hex()} {int(w['combine'])}\n"
    return (head + "".join(c.decode() + "\n" for c in w["contigs"]) + "".join(f"{m} {o}\n" for m, o in w["motifs"]) + "".join(f"{k} {w['table'][k]}\n" for k in keys))


def want_of(w):
    rows, summary = motif_ref.profile(w["contigs"], w["table"], w["code_base"], w["motifs"], w["min_coverage"], w["min_frac"], w["combine"])
    return [(mods_ref.key(c, pos, strand if strand else 1, 0), j, k, a, b, o, f) for c, pos, strand, j, k, a, b, o, f in rows], [tuple(s) for s in summary]


def got_of(exe, w):
    p = subprocess.run([exe, "profile"], input=world_text(w).encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln.split() for ln in p.stdout.decode().splitlines()]
    rows = [tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "R"]
    if w["combine"]:
        rows.sort(key=lambda r: r[:3])                             # (the host walks the segments; the units' order is the device's sort)
    return rows, [tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "S"]


def test_the_tile_is_the_headers(exe):
    assert subprocess.run([exe, "tile"], capture_output=True, check=True).stdout.split() == [str(motif_cases.TILE).encode(), b"31"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case(exe, case):
    assert case["check"](*motif_ref.profile(case["contigs"], case["table"], case["code_base"], case["motifs"], case["min_coverage"], case["min_frac"], case["combine"])), "the case misses its point"
    assert got_of(exe, case) == want_of(case)


@pytest.mark.parametrize("combine", [False, True])
def test_all_in_one(exe, combine):
    w = motif_cases.all_in_one(combine)
    got, want = got_of(exe, w), want_of(w)
    assert got == want and len(want[0]) > 100 and len({r[1] for r in want[0]}) >= 4


@pytest.mark.parametrize("combine", [False, True])
def test_many_units(exe, combine):
    w = motif_cases.many_units(combine)
    got, want = got_of(exe, w), want_of(w)
    assert got == want and len(want[0]) > 8000


def test_refused_items(exe):
    base = dict(contigs=[b"ACGT"], table={}, code_base="C", min_coverage=1, min_frac=0.5)
    for motifs, combine in (([("CG", 2)], False), ([("CN", 1)], False), ([("C" * 33, 0)], False), ([("CG", 0), ("GGTGA", 4)], True), ([("CXG", 0)], False)):
        p = subprocess.run([exe, "profile"], input=world_text(dict(base, motifs=motifs, combine=combine)).encode(), capture_output=True, timeout=300)
        assert p.returncode == 0 and p.stdout.decode() == f"E motif {len(motifs) - 1}\n", motifs
    for m, own in (("GATC", True), ("CCWGG", True), ("GANTC", True), ("CG", True), ("GGTGA", False), ("CCAGG", False), ("RY", True), ("RR", False), ("N", True)):
        assert motif_ref.own_reverse_complement(m) == own, m
