"""The definition of mapDirectly --depth (metamaps_amd/csrc/mm_depth_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the
address and undefined-behaviour sanitizers — against the plain per-position restatement tests/depth_ref.py: the built cases of tests/depth_cases.py (the
wavefront and workgroup edges, 70 000 identical intervals, abutting and nested intervals, a start on another's last + 1, contig ends, a contig of one base,
1 000 contigs with three listed, every window shape, the median's rank around the zeros, no and eight thresholds), 200 random worlds each also with its
intervals permuted, every refusal, and the contig of 2^29 - 1 bases against the values written down by hand.  CPU."""
import os
import random
import subprocess

import pytest

import depth_cases
import depth_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("depth_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_depth_core.cpp")], check=True, timeout=300)
    return p


def world_text(w):
    return (f"W {w['W']} {len(w['lens'])} {len(w['iv'])} {len(w['T'])}\n" + " ".join(str(x) for x in w["lens"]) + "\n" + " ".join(str(x) for x in w["T"]) + "\n"
            + "".join(f"{c} {a} {b}\n" for c, a, b in w["iv"]))


def run(exe, worlds):
    """per world a refusal's words, or a result in depth_ref.profile's shape"""
    p = subprocess.run([exe], input="".join(world_text(w) for w in worlds).encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = []
    cur = dict(runs=[], contig=[], win_off=[], stats=[], win_sum=[], win_covered=[])
    for line in p.stdout.decode().splitlines():
        words = line.split()
        if words[0] == "R":
            out.append(" ".join(words[1:]))
        elif words[0] == "r":
            cur["runs"].append(tuple(int(x) for x in words[1:]))
        elif words[0] == "c":
            cur["contig"].append(int(words[1])); cur["win_off"].append(int(words[2])); cur["stats"].append([int(x) for x in words[3:]])
        elif words[0] == "w":
            cur["win_sum"].append(int(words[1])); cur["win_covered"].append(int(words[2]))
        else:
            assert words[0] == "E"
            cur["win_off"].append(int(words[1]))
            assert len(cur["win_sum"]) == int(words[1])
            out.append(cur)
            cur = dict(runs=[], contig=[], win_off=[], stats=[], win_sum=[], win_covered=[])
    assert len(out) == len(worlds)
    return out


def expected(w):
    return depth_ref.profile(w["lens"], w["iv"], w["W"], w["T"])


def test_built_cases(exe):
    worlds = depth_cases.built_worlds()
    got = dict(zip(worlds, run(exe, list(worlds.values()))))
    for name, w in worlds.items():
        assert got[name] == expected(w), name
    # the restatement itself, by hand
    assert got["abutting"]["runs"] == [(0, 0, 10, 1)] and got["abutting"]["win_sum"] == [5, 5, 0] and got["abutting"]["win_covered"] == [5, 5, 0]
    assert got["coincide"]["runs"] == [(0, 0, 2, 1), (0, 2, 16, 2), (0, 16, 20, 1)]
    assert got["contig_end"]["runs"] == [(0, 5, 9, 1), (0, 9, 10, 2), (1, 0, 1, 2), (1, 1, 4, 1)]
    assert got["length1"]["runs"] == [(0, 0, 1, 1), (2, 0, 1, 2)] and got["length1"]["stats"] == [[1, 1, 1, 1, 1, 1, 0], [2, 1, 2, 2, 2, 1, 1]]
    assert got["three_of_1000"]["contig"] == [7, 500, 998] and got["last_contig"]["contig"] == [2]
    assert got["identical70000"]["runs"] == [(0, 5, 21, 70_000)] and got["identical70000"]["stats"] == [[70_000, 16, 16 * 70_000, 70_000, 70_000, 16, 16, 16, 16, 0]]
    assert got["ladder257"]["stats"][0][4] == 257 and len(got["ladder257"]["runs"]) == 2 * 257 - 1
    assert got["window_over_len"]["win_off"] == [0, 1] and got["window_huge"]["win_sum"] == got["window_is_len"]["win_sum"] == [3 + 1 + 50 + 3 + 30]
    assert got["len_kW"]["win_off"] == [0, 10] and got["len_kW_1"]["win_off"] == [0, 11] and got["len_kW_1"]["win_sum"][-1] == 1 and got["len_kW_1_empty_tail"]["win_sum"][-1] == 0
    assert got["len_kW"]["win_sum"][:3] == [4, 13, 10] and got["window1"]["win_off"] == [0, 100]
    med = lambda name: got[name]["stats"][0][3]
    assert [med(n) for n in ("median_in_zeros_even", "median_last_zero_even", "median_first_covered_even", "median_last_zero_odd", "median_first_covered_odd")] == [0, 0, 1, 0, 1]
    assert med("median_ties") == 2 and med("median_full_cover") == 2
    assert got["no_thresholds"]["stats"] == [[2, 20, 25, 1, 2]] and got["eight_thresholds"]["stats"][0][4] == 18 and got["eight_thresholds"]["stats"][0][-2:] == [14, 0]


def test_200_random_worlds_and_their_permutations(exe):
    worlds = depth_cases.random_worlds()
    assert len(worlds) == 200
    rng = random.Random(7)
    shuffled = [dict(w, iv=rng.sample(w["iv"], len(w["iv"]))) for w in worlds]
    got, again = run(exe, worlds), run(exe, shuffled)
    n_runs = n_multi = 0
    for k, (w, g, h) in enumerate(zip(worlds, got, again)):
        assert g == expected(w), k
        assert h == g, k
        n_runs += len(g["runs"]); n_multi += len(g["contig"]) > 1
    assert n_runs > 3_000 and n_multi > 50, (n_runs, n_multi)


def test_every_refusal(exe):
    good, bad = depth_cases.refused_worlds()
    got = run(exe, [good] + [w for _, w in bad] + [good, dict(good, iv=[])])
    assert got[0] == expected(good) and got[-2] == got[0]
    assert got[1:-2] == [why for why, _ in bad]
    assert got[-1] == dict(runs=[], contig=[], win_off=[0], stats=[], win_sum=[], win_covered=[])
    for why, w in bad:                                               # the restatement refuses the same worlds for the same reason
        assert depth_ref.refused(w["lens"], w["iv"], w["W"], w["T"]) == why, why
    too_many = depth_cases.world([depth_cases.HUGE] * 5, [(c, 0, 0) for c in range(5)], W=1)
    assert run(exe, [too_many]) == ["windows"]                     # 5 * (2^29 - 1) windows of one base


def test_the_contig_of_2_29_minus_1_bases(exe):
    for window in (depth_cases.HUGE, 1000):
        got = run(exe, [depth_cases.huge_world(window)])[0]
        assert got == depth_cases.huge_expected(window), window
    assert len(depth_cases.huge_expected(1000)["win_sum"]) == 536_871 and 70_000 * depth_cases.HUGE > 1 << 32
