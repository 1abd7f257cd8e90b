"""The pileup's definition (metamaps_amd/csrc/mm_pileup_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the address
and undefined-behaviour sanitizers — against the plain restatement tests/pileup_ref.py: the built cases of tests/pileup_cases.py (events at both ends of
a contig, leading and trailing insertions, runs around 64 events, jobs around 64 runs, strand - with N), 200 random jobs, every refusal, and the depth,
threshold and coverage edges of the finish.  CPU."""
import os
import subprocess

import pytest

import pileup_cases
import pileup_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pileup_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_pileup_core.cpp")], check=True, timeout=300)
    return p


def line(j, k, contigs, n_reads=None, **over):
    j = dict(j, **over)
    runs = j["runs"]
    return (f"{j.get('read_index', k)} {k + 1 if n_reads is None else n_reads} {j.get('contig_index', j['c'])} {len(contigs)} {j['strand']} {j['first']} {j['d']} {j.get('use', 1)} "
            f"={j['read'].decode('latin-1')} {len(contigs[j['c']])} {len(runs)} " + " ".join(str(int(w)) for w in runs))


def run(exe, mode, text, n_lines):
    p = subprocess.run([exe, mode], input=text.encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == n_lines
    return out


def check_events(exe, contigs, jobs, names=None):
    got = run(exe, "events", "\n".join(line(j, k, contigs) for k, j in enumerate(jobs)) + "\n", len(jobs))
    for k, (g, j) in enumerate(zip(got, jobs)):
        want = [pileup_ref.key(*e) for e in pileup_ref.events(j)] if pileup_ref.contributes(j) else []
        assert g == (" ".join(str(x) for x in want) if want else "-"), (k, names[k] if names else None, j["strand"], j["first"], [(w >> 4, w & 15) for w in j["runs"]][:12])
    return got


def test_built_cases(exe):
    contigs, jobs = pileup_cases.built_world()
    got = dict(zip(jobs, check_events(exe, contigs, list(jobs.values()), list(jobs))))
    K, n0 = pileup_ref.key, len(contigs[0])
    assert got["eq_only"] == "-" and got["not_used"] == "-" and got["not_aligned"] == "-" and got["empty_read"] == "-" and got["runs0"] == "-"
    assert pileup_ref.unkey(int(got["x_at_0"]))[:2] == (0, 0) and pileup_ref.unkey(int(got["x_at_end"]))[:2] == (0, n0 - 1)
    assert got["lead_i"] == str(K(0, 30, 6)) and got["trail_i"] == str(K(0, 39, 6)) and got["i_at_len"] == str(K(0, n0 - 1, 6)) and got["only_i"] == str(K(1, 5, 6))
    for n in (1, 63, 64, 65, 200):
        assert got[f"d{n}"].split() == [str(K(1, 8 + t, 5)) for t in range(n)]
    codes = [pileup_ref.unkey(int(x))[2] for x in got["x70_rev_n"].split()]
    assert len(codes) == 70 and codes.count(4) == 2 and codes[11] == 4 and codes[66] == 4
    assert got["twice_a"] == got["twice_b"] and pileup_ref.unkey(int(got["same_pos_c0"])) == (0, 285, 5) and pileup_ref.unkey(int(got["same_pos_c1"])) == (1, 285, 5)
    assert len(got["runs129"].split()) == 64 and len(got["long_then_short"].split()) == 90 + 1 + 66 + 1 + 65 + 2


def test_200_random_jobs(exe):
    contigs, jobs = pileup_cases.random_world()
    assert len(jobs) == 200 and {j["strand"] for j in jobs} == {1, -1} and {j["c"] for j in jobs} == {0, 1, 2}
    assert {w & 15 for j in jobs for w in j["runs"]} == {1, 2, 7, 8} and max(w >> 4 for j in jobs for w in j["runs"] if w & 15 in (2, 8)) > 64
    assert sum(not pileup_ref.contributes(j) for j in jobs) > 20
    got = check_events(exe, contigs, jobs)
    codes = {pileup_ref.unkey(int(x))[2] for g in got if g != "-" for x in g.split()}
    assert codes == {0, 1, 2, 3, 4, 5, 6}


def test_every_rule(exe):
    contigs, _ = pileup_cases.built_world()
    cases = pileup_cases.broken_jobs(contigs)
    lines = []
    for j, over, rule in cases:
        over = dict(over)
        idx = {k + "_index": over.pop(k) for k in ("read", "contig") if k in over}
        lines.append(line(dict(j, **idx), 0, contigs, 1, **over))
    assert run(exe, "events", "\n".join(lines) + "\n", len(lines)) == [f"E {rule}" for _, _, rule in cases]
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]
    # rule 7 is not the pileup's: a dist that disagrees with the runs still contributes; a broken job that is not used is not looked at
    base = cases[0][0]
    got = run(exe, "events", line(base, 0, contigs, d=99) + "\n" + line(base, 0, contigs, use=0, strand=0) + "\n", 2)
    assert got[0] == " ".join(str(pileup_ref.key(*e)) for e in pileup_ref.events(base)) and got[1] == "-"


@pytest.mark.parametrize("world", pileup_cases.finish_worlds(), ids=lambda w: w[0])
def test_finish(exe, world):
    name, clen, t, iv, min_count, min_frac = world
    sites, contigs = pileup_ref.finish(t, iv, clen, min_count, min_frac)
    text = f"{min_count} {min_frac!r} {len(clen)} {len(t)} {len(iv)}\n" + "".join(f"{k} {t[k]}\n" for k in sorted(t)) + "".join(f"{c} {a} {b}\n" for c, a, b in iv)
    got = run(exe, "finish", text, len(sites) + len(clen))
    assert got == [f"S {k} {n} {d}" for k, n, d in sites] + [f"C {a} {c} {s}" for a, c, s in contigs]
    if name == "edges":                                            # the restatement itself, by hand
        assert contigs == [(6, 51, 65), (0, 0, 0), (3, 40, 60), (1, 7, 7)] and [d for _, _, d in sites] == [1, 1, 1, 2, 2, 2, 1, 1, 1]
    if name == "count_eq_min_count":
        assert [n for _, n, _ in sites] == [3, 2]
    if name == "frac_half":
        assert [(n, d) for _, n, d in sites] == [(2, 4), (2, 3)]
