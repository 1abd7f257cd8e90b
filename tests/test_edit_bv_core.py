"""The block form of Myers' bit-vector recurrence and its 64-lane systolic schedule (metamaps_amd/csrc/mm_edit_bv_core.hpp), built for the host with
g++ — plain, and as a stand-alone program under the address and undefined-behaviour sanitizers — in both forms, the serial one and the pipeline of 64
emulated lanes, against the naive dynamic programme (tests/edit_ref.py): the edge cases, d == cap and d == cap + 1, 500 random problems, the ladder of
read lengths at which a lane gets another block, and windows shorter than the pipeline.  Every comparison is exact.  CPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_bv_cases
import edit_cases
import edit_ref

HERE = os.path.dirname(os.path.abspath(__file__))
W = edit_bv_cases.W


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("edit_bv") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_edit_bv_core.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def wanted():
    """the reference's answers, computed once per problem list"""
    memo = {}

    def get(name, problems):
        if name not in memo:
            memo[name] = [edit_ref.infix(r, s, w, md) for r, s, w, md in problems]
        return memo[name]
    return get


def run(exe, lines):
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def align(exe, form, problems):
    big = 1 << 30
    lines = [f"{form} {s} {big if md is None else md} ={r.decode('latin-1')} ={w.decode('latin-1')}" for r, s, w, md in problems]
    got = []
    for line in run(exe, lines):
        d, a, b = (int(x) for x in line.split())
        got.append(None if d < 0 else (d, a, b))
    return got


def check(exe, form, problems, want):
    got = align(exe, form, problems)
    for k, (g, x) in enumerate(zip(got, want)):
        assert g == x, (form, k, problems[k][1], len(problems[k][0]), len(problems[k][2]), problems[k][3], g, x)
    return got


FORMS = pytest.mark.parametrize("form", ["S", "P"], ids=["serial", "pipeline"])


@FORMS
def test_edges(exe, form, wanted):
    problems = edit_cases.edge_problems(np.random.default_rng(7))
    got = check(exe, form, problems, wanted("edges", problems))
    assert got[32:35] == [(20, 0, 0), None, (0, 0, 0)]             # an empty window
    assert got[-3] == (4, 2, 18) and got[-2] == (4, 0, 0) and got[-1] == (2, 2, 12)      # N matches nothing; lower case matches; IUPAC matches nothing
    pair = list(edit_cases.at_cap_pair(np.random.default_rng(8)))
    assert check(exe, form, pair, wanted("cap", pair)) == [(5, 20, 80), None]           # d == cap is aligned, d == cap + 1 is not


@FORMS
def test_500_random_problems(exe, form, wanted):
    rng = np.random.default_rng(52)
    problems = [edit_cases.random_problem(rng, k) for k in range(500)]
    got = check(exe, form, problems, wanted("random", problems))
    assert sum(g is None for g in got) > 20 and sum(g is not None and g[0] > 0 for g in got) > 200


@FORMS
def test_block_ladder(exe, form, wanted):
    problems = edit_bv_cases.ladder_problems(np.random.default_rng(61))
    assert sorted({len(p[0]) for p in problems}) == [0, 1, W - 1, W, W + 1, 64 * W - 1, 64 * W, 64 * W + 1, 128 * W + 1]
    got = check(exe, form, problems, wanted("ladder", problems))
    assert sum(g is not None and g[0] > 100 for g in got) >= 6 and sum(p[1] < 0 for p in problems) == len(problems) // 2


@FORMS
def test_window_shorter_than_the_pipeline(exe, form, wanted):
    problems = edit_bv_cases.short_window_problems(np.random.default_rng(62))
    assert [len(p[2]) for p in problems[::2]] == [0, 1, 63, 64, 65] and all(len(p[0]) > 64 * W for p in problems)
    check(exe, form, problems, wanted("short", problems))


def test_lane_partition(exe):
    """blocks, blocks per lane, register class and the lane of the last block at the edges of the ladder and at the longest read"""
    ms = [0, 1, W, W + 1, 64 * W, 64 * W + 1, 128 * W, 128 * W + 1, 10000, 65536]
    got = [tuple(int(x) for x in line.split()) for line in run(exe, [f"B {m}" for m in ms])]
    assert got == [(0, 0, 1, 0), (1, 1, 1, 0), (1, 1, 1, 0), (2, 1, 1, 1), (64, 1, 1, 63), (65, 2, 2, 32), (128, 2, 2, 63), (129, 3, 4, 42), (313, 5, 8, 62), (2048, 32, 32, 63)]
