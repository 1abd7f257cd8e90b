"""The definition of mapDirectly --error-profile (metamaps_amd/csrc/mm_errprof_core.hpp), built for the host with g++ — plain, and as a stand-alone program
under the address and undefined-behaviour sanitizers — against the plain per-column restatement tests/errprof_ref.py: the built cases of
tests/errprof_cases.py one by one and together (tile edges, the all-lanes path of every op, the bin cap, indels at both ends of a contig, N on either side,
both strands with asymmetric qualities, qualities 0 and 93, reads without), 200 random jobs, every rule, and a few values written down by hand.  CPU."""
import os
import subprocess

import pytest

import errprof_cases
import errprof_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("errprof_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_errprof_core.cpp")], check=True, timeout=300)
    return p


def line(j, contigs, **over):
    """the job as the driver reads it: its read and its contig sit at their own indexes of sets that hold nothing else"""
    j = dict(j, **{k: v for k, v in over.items() if k in ("strand", "first", "runs")})
    qual = "-" if j.get("qual") is None else "".join("%02x" % q for q in j["qual"])
    words = [over.get("read", 0), 1, over.get("contig", j["c"]), len(contigs), j["strand"], j["first"], j["d"], j.get("use", 1), "=" + j["read"].decode("latin-1"), "=" + qual,
             "=" + contigs[j["c"]].decode("latin-1"), len(j["runs"])] + list(j["runs"])
    return " ".join(str(w) for w in words) + "\n"


def run(exe, text):
    """(counters, per job its columns and key, or ("E", rule))"""
    p = subprocess.run([exe], input=text.encode("latin-1"), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rows, counters = [], None
    for ln in p.stdout.decode().splitlines():
        w = ln.split()
        if w[0] == "J":
            rows.append(([int(x) for x in w[1:7]], int(w[7])))
        elif w[0] == "E":
            rows.append(("E", int(w[1])))
        else:
            assert w[0] == "T"
            counters = [int(x) for x in w[1:]]
    return counters, rows


def same(got, want):
    counters, cols, keys = want
    assert got[0] == counters
    assert [c for c, _ in got[1]] == cols and [k for _, k in got[1]] == keys


def test_built_cases(exe):
    contigs, jobs = errprof_cases.built_world()
    for name, j in jobs.items():                                    # one by one
        got = run(exe, line(j, contigs))
        assert got[0] == errprof_ref.profile([j], contigs)[0], name
        same(got, errprof_ref.profile([j], contigs))
    all_jobs = list(jobs.values())
    got = run(exe, "".join(line(j, contigs) for j in all_jobs))
    want = errprof_ref.profile(all_jobs, contigs)
    same(got, want)
    # the restatement itself, by hand
    one = lambda name: errprof_ref.profile([jobs[name]], contigs)
    t = errprof_ref.unflat(one("one_eq_f")[0])
    assert sum(map(sum, t["sub"])) == 1 and t["qual"][0][94] == 1 and one("one_eq_f")[1] == [[1, 0, 0, 0, 0, 0]] and one("one_eq_f")[2] == [1_000_000]
    for name, kind, hp, bin_ in (("i63_f", 0, 0, 62), ("i64_r", 0, 0, 63), ("i65_f", 0, 0, 63), ("d65_r", 1, None, 63), ("i65_in_g_f", 0, 1, 63), ("i65_last_breaks_r", 0, 0, 63),
                                 ("i64_first_breaks_f", 0, 0, 63), ("i3_has_n_f", 0, 0, 2), ("d63_of_g_r", 1, 1, 62), ("d70_whole_g_f", 1, 0, 63), ("d2_mixed_f", 1, 0, 1),
                                 ("i_g_before_g_f", 0, 1, 1), ("i_g_behind_g_r", 0, 1, 1), ("lead_i_at_0_f", 0, 1, 1), ("d_at_0_r", 1, 1, 2), ("d_to_last_base_f", 1, 1, 2),
                                 ("i_after_last_base_r", 0, 1, 1)):
        ind = errprof_ref.unflat(one(name)[0])["indel"]
        if hp is not None:
            assert ind[kind][hp][bin_] == 1, name
        assert sum(ind[kind][0]) + sum(ind[kind][1]) == 1 and ind[kind][0][bin_] + ind[kind][1][bin_] == 1, name
    t = errprof_ref.unflat(one("n_in_read_x_f")[0])
    assert sum(t["sub"][a][4] for a in range(5)) == 2                # two read bytes outside A C G T
    t = errprof_ref.unflat(one("n_in_ref_eq_r")[0])
    assert t["sub"][4][4] == 2 and sum(t["sub"][4]) == 2            # N under N, n under n
    t = errprof_ref.unflat(one("q0_and_93")[0])
    assert sum(t["qual"][s][0] for s in range(3)) == 8 and sum(t["qual"][s][93] for s in range(3)) == 7 and sum(t["qual"][s][94] for s in range(3)) == 0
    f, r = one("x65_f"), one("x65_r")
    assert f[1] == r[1] == [[4, 65, 0, 0, 0, 0]] and f[2] == r[2] == [1 << 32 | (4_000_000 // 69)]
    # strand -1 counts in the read's orientation: the complemented cells of strand +1
    tf, tr = errprof_ref.unflat(f[0])["sub"], errprof_ref.unflat(r[0])["sub"]
    assert all(tf[a][b] == tr[3 - a][3 - b] for a in range(4) for b in range(4)) and tf != tr
    for name in ("not_used", "not_aligned"):
        assert one(name) == ([0] * 566, [[0] * 6], [errprof_ref.NO_KEY]), name
    assert one("empty_read") == ([0] * 566, [[0] * 6], [0])


def test_200_random_jobs(exe):
    contigs, jobs = errprof_cases.random_world()
    assert len(jobs) == 200 and max(sum(int(w) >> 4 for w in j["runs"]) for j in jobs) <= 300
    want = errprof_ref.profile(jobs, contigs)
    same(run(exe, "".join(line(j, contigs) for j in jobs)), want)
    t = errprof_ref.unflat(want[0])
    cols = want[1]
    assert sum(t["sub"][a][a] for a in range(5)) < sum(map(sum, t["sub"])) == sum(c[0] + c[1] for c in cols)
    assert sum(t["qual"][0]) == sum(c[0] for c in cols) and sum(t["qual"][1]) == sum(c[1] for c in cols) and sum(t["qual"][2]) == sum(c[3] for c in cols)
    assert sum(map(sum, t["indel"][0])) == sum(c[2] for c in cols) and sum(map(sum, t["indel"][1])) == sum(c[4] for c in cols)
    assert all(sum(t["indel"][k][h]) > 20 for k in range(2) for h in range(2)) and t["indel"][0][0][63] + t["indel"][0][1][63] > 0   # the world is not degenerate
    assert sum(t["qual"][0][:94]) > 1000 and t["qual"][0][94] > 1000 and all(t["sub"][a][b] > 0 for a in range(4) for b in range(5))


def test_every_rule(exe):
    contigs, jobs = errprof_cases.built_world()
    good = jobs["x65_f"]
    cases = errprof_cases.broken_jobs(contigs)
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]
    for j, over, rule in cases:
        got = run(exe, line(good, contigs) + line(j, contigs, **over))
        assert got[1][1] == ("E", rule), (over, rule)
        assert got[0] == errprof_ref.profile([good], contigs)[0]      # the broken job has added nothing
    # a job that is not used is not checked
    got = run(exe, line(dict(cases[0][0], use=0), contigs, strand=0))
    assert got == ([0] * 566, [([0] * 6, errprof_ref.NO_KEY)])
