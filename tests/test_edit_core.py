"""The definition of the exact edit distances of mappings, the packed strings, the two-pass wavefront alignment and the checks on a job's
arguments (metamaps_amd/csrc/mm_edit_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the address and
undefined-behaviour sanitizers — against the naive dynamic programme (tests/edit_ref.py): the edge cases, 500 random problems, the window and cap
rules and the refusal codes.  Every comparison is exact.  CPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_cases
import edit_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("edit") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_edit_core.cpp")], check=True, timeout=300)
    return p


def run(exe, lines):
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def align(exe, problems):
    big = 1 << 30
    lines = [f"A {s} {big if md is None else md} ={r.decode('latin-1')} ={w.decode('latin-1')}" for r, s, w, md in problems]
    got = []
    for line in run(exe, lines):
        d, a, b = (int(x) for x in line.split())
        got.append(None if d < 0 else (d, a, b))
    return got


def check(exe, problems):
    got = align(exe, problems)
    want = [edit_ref.infix(r, s, w, md) for r, s, w, md in problems]
    for k, (g, x) in enumerate(zip(got, want)):
        assert g == x, (k, problems[k], g, x)
    return got


def test_edges(exe):
    rng = np.random.default_rng(7)
    problems = edit_cases.edge_problems(rng)
    got = check(exe, problems)
    assert [p[2] for p in problems[32:35]] == [b"", b"", b""] and got[32:35] == [(20, 0, 0), None, (0, 0, 0)]      # an empty window
    hit, miss = edit_cases.at_cap_pair(np.random.default_rng(8))
    assert check(exe, [hit, miss]) == [(5, 20, 80), None]           # d == cap is aligned, d == cap + 1 is not
    assert got[-3] == (4, 2, 18)                                    # four N against four N are four substitutions; lower case matches
    assert got[-2] == (4, 0, 0)                                     # N against N: nothing matches, the empty substring at the smallest end
    assert got[-1] == (2, 2, 12)                                    # the IUPAC bytes and their complements match nothing


def test_500_random_problems(exe):
    rng = np.random.default_rng(52)
    problems = [edit_cases.random_problem(rng, k) for k in range(500)]
    got = check(exe, problems)
    assert sum(g is None for g in got) > 20 and sum(g is not None and g[0] > 0 for g in got) > 200
    assert sum(p[1] < 0 for p in problems) > 100 and sum(g is not None and g[0] == 0 for g in got) > 20


def test_window_and_cap_rules(exe):
    cases = [(s, L, C) for L in (0, 1, 15, 16, 1000, 65536) for C in (0, 1, 100, 5000) for s in (-5, 0, 1, 63, 64, 65, 99, 100, 4999, 5000, 7000)]
    got = run(exe, [f"W {s} {L} {C}" for s, L, C in cases])
    for line, (s, L, C) in zip(got, cases):
        assert tuple(int(x) for x in line.split()) == edit_ref.window(s, L, C), (s, L, C)
    assert edit_ref.window(100, 1000, 5000) == (0, 1226) and edit_ref.window(4500, 1000, 5000) == (4374, 5000)
    caps = [(L, pi) for L in (0, 1, 3, 10, 99, 100, 1001, 2500, 65536) for pi in (80.0, 90.0, 70.0, 85.5, 100.0, 0.0)]
    got = run(exe, [f"C {L} {pi}" for L, pi in caps])
    for line, (L, pi) in zip(got, caps):
        assert int(line) == edit_ref.cap(L, pi), (L, pi)
    assert [edit_ref.cap(L) for L in (10, 99, 100, 1001)] == [3, 29, 30, 300]      # floor(0.3 L) at the default --pi


def test_records(exe):
    rng = np.random.default_rng(53)
    contig = edit_cases.dna(rng, 3000)
    rows = []
    for start, L, strand, rate, over in [(0, 200, 1, 0.05, 0), (1000, 500, -1, 0.1, 0), (2790, 200, 1, 0.02, 0), (2900, 100, -1, 0.0, 30), (1500, 400, 1, 0.6, 0)]:
        read = edit_cases.mutate(rng, contig[start:start + L], rate) + edit_cases.dna(rng, over)
        rows.append((edit_cases.stored(read, strand), strand, start + int(rng.integers(-30, 30))))
    got = run(exe, [f"R {s} 80 {st} ={r.decode()} ={contig.decode()}" for r, s, st in rows])
    want = [edit_ref.record(r, s, contig, st) for r, s, st in rows]
    assert [None if g == "NA" else tuple(int(x) for x in g.split()) for g in got] == want
    assert want[-1] is None and want[0][1] <= 2 and 0 < want[3][0] <= 30 and want[3][2] <= 2999      # windows clamped at both ends of the contig; a read that hangs over


def test_refusals(exe):
    ok = [1, 1, 0, 5, 10, 90, 3, 2]                                 # read strand contig max_dist ws we n_reads n_contigs; contig lengths 100, 50
    change = lambda k, v: ok[:k] + [v] + ok[k + 1:]
    cases = [(ok, 0), (change(0, 3), 1), (change(0, -1), 1), (change(2, 2), 2), (change(2, -1), 2), (change(1, 0), 3), (change(1, 2), 3), (change(3, -1), 4),
             (change(5, 9), 5), (change(5, 101), 5), (change(4, -1), 5), (change(5, 100), 0), (change(5, 10), 0), (change(3, 0), 0), (change(1, -1), 0),
             ([1, 1, 1, 5, 10, 51, 3, 2], 5)]
    got = run(exe, ["K " + " ".join(map(str, c)) + " 100 50" for c, _ in cases])
    assert [int(g) for g in got] == [code for _, code in cases]
