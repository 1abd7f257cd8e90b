"""The storing pass of the bit-vector recurrence and the walk back through it (metamaps_amd/csrc/mm_edit_trace_core.hpp), built for the host with g++
— plain, and as a stand-alone program under the address and undefined-behaviour sanitizers — in both forms, the serial one and the pipeline of 64
emulated lanes, against the naive suffix table and its walk (tests/edit_cigar_ref.py): the edge cases, d == cap and d == cap + 1, 500 random
problems, the ladder of read lengths at which a lane gets another block, windows shorter than the pipeline, and the built cases (a long insertion,
a long deletion, both across the row between two lanes, an exact match).  (d, a, b, runs) compare exactly; the invariants of the definition are
checked on every answer without the reference.  CPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_bv_cases
import edit_cases
import edit_cigar_ref
import edit_trace_cases

HERE = os.path.dirname(os.path.abspath(__file__))
W = edit_bv_cases.W


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("edit_trace") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_edit_trace_core.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def wanted():
    """the reference's answers, computed once per problem list"""
    memo = {}

    def get(name, problems):
        if name not in memo:
            memo[name] = [edit_cigar_ref.align(r, s, w, md) for r, s, w, md in problems]
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
        v = [int(x) for x in line.split()]
        assert v[3] == len(v) - 4, "the walk counted the runs it wrote"
        got.append(None if v[0] < 0 else (v[0], v[1], v[2], v[4:]))
    return got


def check(exe, form, problems, want):
    got = align(exe, form, problems)
    for k, (g, x) in enumerate(zip(got, want)):
        where = (form, k, problems[k][1], len(problems[k][0]), len(problems[k][2]), problems[k][3])
        assert (g is None) == (x is None) and (g is None or g[:3] == x[:3]), where + (g and g[:3], x and x[:3])
        if g is not None:
            assert g[3] == x[3], where + (edit_cigar_ref.cigar(g[3])[:300], edit_cigar_ref.cigar(x[3])[:300])
            edit_cigar_ref.check_invariants(*problems[k][:3], g)
    return got


FORMS = pytest.mark.parametrize("form", ["S", "P"], ids=["serial", "pipeline"])


@FORMS
def test_edges(exe, form, wanted):
    problems = edit_cases.edge_problems(np.random.default_rng(7))
    got = check(exe, form, problems, wanted("edges", problems))
    assert got[32:35] == [(20, 0, 0, [20 << 4 | 1]), None, (0, 0, 0, [])]          # an empty window: 20I; an empty read: no run
    assert [edit_cigar_ref.cigar(g[3]) for g in got[-3:]] == ["4=4X8=", "4I", "4=2X4="]   # N matches nothing; lower case matches; IUPAC matches nothing
    pair = list(edit_cases.at_cap_pair(np.random.default_rng(8)))
    got = check(exe, form, pair, wanted("cap", pair))
    assert got[1] is None and edit_cigar_ref.cigar(got[0][3]) == "5=1X11=1X11=1X11=1X11=1X6="


@FORMS
def test_500_random_problems(exe, form, wanted):
    rng = np.random.default_rng(52)
    problems = [edit_cases.random_problem(rng, k) for k in range(500)]
    got = check(exe, form, problems, wanted("random", problems))
    assert sum(g is None for g in got) > 20 and sum(g is not None and g[0] > 0 for g in got) > 200
    ops = {w & 15 for g in got if g for w in g[3]}
    assert ops == {1, 2, 7, 8}


@FORMS
def test_block_ladder(exe, form, wanted):
    problems = edit_bv_cases.ladder_problems(np.random.default_rng(61))
    assert sorted({len(p[0]) for p in problems}) == [0, 1, W - 1, W, W + 1, 64 * W - 1, 64 * W, 64 * W + 1, 128 * W + 1]
    got = check(exe, form, problems, wanted("ladder", problems))
    assert sum(g is not None and len(g[3]) > 100 for g in got) >= 6


@FORMS
def test_window_shorter_than_the_pipeline(exe, form, wanted):
    problems = edit_bv_cases.short_window_problems(np.random.default_rng(62))
    assert [len(p[2]) for p in problems[::2]] == [0, 1, 63, 64, 65] and all(len(p[0]) > 64 * W for p in problems)
    check(exe, form, problems, wanted("short", problems))


@FORMS
def test_built_cases(exe, form, wanted):
    """an insertion of 100 bases (the walk climbs through more than two blocks in one column), a deletion of 150 (it crosses a strip of 64 columns
    inside one block), both across a row where one lane's blocks end and the next one's begin (tests/edit_trace_cases.py says which and why), and
    an exact match on either strand"""
    problems = edit_trace_cases.built_problems(np.random.default_rng(63))
    want = wanted("built", problems)
    edit_trace_cases.check_built(problems, want)
    check(exe, form, problems, want)


def test_scratch_words(exe):
    """(n + 63) steps of 64 lanes, two words per block of a lane; nothing for an empty read or an empty stretch"""
    got = [int(x) for x in run(exe, ["W 0 10", "W 10 0", "W 1 1", "W 2048 100", "W 2049 100", "W 10000 10600", "W 65536 70000"])]
    assert got == [0, 0, 64 * 64 * 2, 163 * 64 * 2, 163 * 64 * 4, 10663 * 64 * 10, 70063 * 64 * 64]


def test_launch_plan(exe):
    """jobs cut into launches whose scratch fits the budget, one job at least per launch (the budget is raised to the largest job), at most max_jobs
    per launch; a job that is not aligned, an empty read and a read beyond the longest take no scratch and no slot"""
    jobs = [(100, 3, 5, 105), (100, -1, -1, -1), (0, 0, 0, 0), (3000, 40, 0, 2990), (100, 0, 10, 110), (65537, -1, -1, -1), (2049, 7, 1, 2001)]
    w = [int(x) for x in run(exe, [f"W {m} {b - a}" for m, d, a, b in jobs])]
    w = [x if d >= 0 and 0 < m <= 65536 else 0 for x, (m, d, a, b) in zip(w, jobs)]
    slot = [2 * d + 1 if x else 0 for x, (m, d, a, b) in zip(w, jobs)]
    assert w[0] == 163 * 64 * 2 and w[3] == 3053 * 64 * 4 and [x > 0 for x in w] == [True, False, False, True, True, False, True]
    flat = " ".join(f"{m} {d} {a} {b}" for m, d, a, b in jobs)

    def plan(budget, max_jobs=1 << 30):
        head, cut, scr, slots = run(exe, [f"L {budget} {max_jobs} {len(jobs)} {flat}"])[0].split("|")
        return [int(x) for x in head.split()], [int(x) for x in cut.split()], [int(x) for x in scr.split()], [int(x) for x in slots.split()]

    slot_off = [sum(slot[:k]) for k in range(len(jobs))]
    head, cut, scr, slots = plan(1 << 40)                           # everything in one launch
    assert head == [1, sum(w), sum(slot)] and cut == [0, 7] and scr == [sum(w[:k]) for k in range(7)] and slots == slot_off
    head, cut, scr, slots = plan(1)                                 # a budget below every job: a launch per job that needs scratch
    assert cut == [0, 3, 4, 6, 7] and head == [4, max(w), sum(slot)] and scr == [0, w[0], w[0], 0, 0, w[4], 0] and slots == slot_off
    head, cut, scr, slots = plan(w[0] + w[3])                       # the first four fit exactly; the rest is smaller than that
    assert w[4] + w[6] < w[0] + w[3] and cut == [0, 4, 7] and head == [2, w[0] + w[3], sum(slot)] and scr == [0, w[0], w[0], w[0], 0, w[4], w[4]] and slots == slot_off
    head, cut, scr, slots = plan(1 << 40, 2)                        # at most two jobs per launch
    assert cut == [0, 2, 4, 6, 7] and head[0] == 4
    assert plan(5)[0][0] == 4 and run(exe, ["L 100 10 0"])[0].split("|")[0].split() == ["1", "0", "0"]   # no job: one empty launch, nothing to allocate
