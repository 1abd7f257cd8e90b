"""The definition of mapDirectly --vcf's alleles (metamaps_amd/csrc/mm_vcf_core.hpp), built for the host with g++ — plain, and as a stand-alone program under
the address and undefined-behaviour sanitizers — against the plain restatement tests/vcf_ref.py: the built cases of tests/vcf_cases.py (indels at the ends of
an alignment, shifts that stop at `first`, at position 0, at an N and after 256 steps, insertions that turn inside tandem repeats, indels of 24 and 25 bases,
N among alts and inserted bases, X runs around 64 bases, jobs around 64 runs, both strands), 200 random jobs on low-complexity contigs, every refusal, and the
depth, threshold and window edges of the finish.  CPU."""
import os
import subprocess

import pytest

import vcf_cases
import vcf_ref

HERE = os.path.dirname(os.path.abspath(__file__))
K = vcf_ref.key


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vcf_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_vcf_core.cpp")], check=True, timeout=300)
    return p


def line(j, k, contigs, n_reads=None, **over):
    j = dict(j, **over)
    runs = j["runs"]
    return (f"{j.get('read_index', k)} {k + 1 if n_reads is None else n_reads} {j.get('contig_index', j['c'])} {len(contigs)} {j['strand']} {j['first']} {j['d']} {j.get('use', 1)} "
            f"={j['read'].decode('latin-1')} ={contigs[j['c']].decode('latin-1')} {len(runs)} " + " ".join(str(int(w)) for w in runs))


def run(exe, mode, text, n_lines):
    p = subprocess.run([exe, mode], input=text.encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == n_lines
    return out


def bound(j):
    """the alleles a job has room for: its X bases and its I and D runs that are neither first nor last"""
    runs = j["runs"]
    return sum(w >> 4 for w in runs if w & 15 == 8) + sum(1 for k, w in enumerate(runs) if w & 15 in (1, 2) and 0 < k < len(runs) - 1)


def check_events(exe, contigs, jobs, names=None):
    """every job's alleles against the restatement; returns them per job as [(w0, w1)]"""
    got = run(exe, "events", "\n".join(line(j, k, contigs) for k, j in enumerate(jobs)) + "\n", len(jobs))
    out = []
    for k, (g, j) in enumerate(zip(got, jobs)):
        what = (k, names[k] if names else None, j["strand"], j["first"], [(w >> 4, w & 15) for w in j["runs"]][:12])
        want = [K(e) for e in vcf_ref.alleles(j, contigs)] if vcf_ref.contributes(j) else []
        words = [] if g == "-" else g.split()
        assert len(words) == (bound(j) if vcf_ref.contributes(j) else 0), what
        mine = [tuple(int(x) for x in w.split(":")) for w in words if w != "skip"]
        assert mine == want, what
        out.append(mine)
    return out


def test_built_cases(exe):
    contigs, jobs = vcf_cases.built_world()
    got = dict(zip(jobs, check_events(exe, contigs, list(jobs.values()), list(jobs))))
    hp, di, hand, hpn, hp300 = vcf_cases.HP12[1], vcf_cases.DI10[1], vcf_cases.HAND[1], vcf_cases.HP_N[1], vcf_cases.HP300[1]
    for tag in "fr":                                                # the restatement itself, by hand
        for name in ("eq_only", "lead_i", "trail_i", "lead_d", "trail_d", "lead_i_then_d", "d_then_trail_i", "only_i", "i_with_n"):
            assert got[f"{name}_{tag}"] == [], name
        assert got[f"hp_to_first_d_{tag}"] == [K((0, hp + 2, "D", 1))] and got[f"hp_to_first_i_{tag}"] == [K((0, hp + 3, "I", "AA"))]
        assert got[f"hp_whole_d_{tag}"] == [K((0, hp - 1, "D", 2))]
        assert got[f"at_0_d_{tag}"] == [K((0, 0, "D", 1))] and got[f"at_0_i_{tag}"] == [K((0, 0, "I", "T"))]
        assert got[f"n_stops_d_{tag}"] == [K((0, hpn + 4, "D", 1))] and got[f"n_stops_i_{tag}"] == [K((0, hpn + 4, "I", "A"))]   # the N at hpn + 4 is the anchor
        assert got[f"hand_rot_{tag}"] == [K((0, hand, "I", "AC"))]
        assert got[f"di_ins_1_5_{tag}"][0][0] >> 3 & 0xFFFFFFFF < di + 15 and got[f"tri_ins_1_5_{tag}"] != []
        # a = first + k has k steps to `first`; 256 are taken at most
        assert [got[f"steps{k}_d_{tag}"] for k in (255, 256, 257)] == [[K((1, 25, "D", 1))], [K((1, 25, "D", 1))], [K((1, 26, "D", 1))]]
        assert [got[f"steps{k}_i_{tag}"] for k in (255, 256, 257)] == [[K((1, 25, "I", "AA"))], [K((1, 25, "I", "AA"))], [K((1, 26, "I", "AA"))]]
        assert got[f"d24_{tag}"][0][1] == 24 and got[f"d25_{tag}"][0][1] == 25
        assert got[f"i24_{tag}"][0][1] >> 48 == 24 and got[f"i24_{tag}"][0][1] & (1 << 48) - 1 != 0 and got[f"i25_{tag}"][0][1] == 25 << 48
        assert [k[0] & 7 for k in got[f"x_n_between_{tag}"]] == [2, 2] and len(got[f"x64_{tag}"]) == 64 and len(got[f"x65_{tag}"]) == 65 and len(got[f"x70_n_{tag}"]) == 68
        assert len(got[f"runs129_{tag}"]) == 22 + 21 + 21 and hp300 == 20
    assert got["same_del_a"] == got["same_del_b"] == [K((0, hp - 1, "D", 1))]
    assert got["not_used"] == [] and got["not_aligned"] == [] and got["empty_read"] == []
    assert vcf_ref.table([jobs["same_del_a"], jobs["same_del_b"]], contigs) == {K((0, hp - 1, "D", 1)): 2}


def test_200_random_jobs(exe):
    contigs, jobs = vcf_cases.random_world()
    assert len(jobs) == 200 and {j["strand"] for j in jobs} == {1, -1} and {j["c"] for j in jobs} == {0, 1}
    assert sum(not vcf_ref.contributes(j) for j in jobs) > 20
    got = check_events(exe, contigs, jobs)
    flat = [k for g in got for k in g]
    assert {k[0] & 7 for k in flat} == {0, 1, 2, 3, 5, 6}
    assert any(k[0] & 7 == 6 and k[1] >> 48 > 24 for k in flat) and any(k[0] & 7 == 5 and k[1] > 24 for k in flat)
    # indels did move, some of them by the full 256 steps, and insertions did turn
    moved = turned = full = 0
    for j in jobs:
        if not vcf_ref.contributes(j):
            continue
        raw = dict(j)
        r, i = j["first"], 0
        q = vcf_ref.pileup_ref.oriented(j["read"], j["strand"])
        norm = {(e[2], e[3] if e[2] == "D" else len(e[3])): e for e in vcf_ref.alleles(j, contigs) if e[2] != "S"}
        for w in raw["runs"]:
            n, op = w >> 4, w & 15
            e = norm.get(("D", n) if op == 2 else ("I", n)) if op in (1, 2) else None
            if e is not None and e[1] < r - 1:
                moved += 1
                full += e[1] == r - 1 - vcf_ref.NORM_MAX
                turned += op == 1 and e[3] != "".join(q[i:i + n])
            r += n if op != 1 else 0
            i += n if op != 2 else 0
    assert moved > 50 and turned > 3, (moved, turned, full)


def test_every_rule(exe):
    contigs, _ = vcf_cases.built_world()
    contigs = contigs + [vcf_cases.big_contig()]
    cases = vcf_cases.broken_jobs(contigs)
    lines = []
    for j, over, rule in cases:
        over = dict(over)
        idx = {k + "_index": over.pop(k) for k in ("read", "contig") if k in over}
        lines.append(line(dict(j, **idx), 0, contigs, 1, **over))
    assert run(exe, "events", "\n".join(lines) + "\n", len(lines)) == [f"E {rule}" for _, _, rule in cases]
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6, 8]
    # rule 7 is not ours: a dist that disagrees with the runs still contributes; a broken job that is not used is not looked at; a run of 2^16 - 1 bases,
    # and one of 2^16 that leads the alignment, pass
    base, big = cases[0][0], cases[-1][0]
    ok = vcf_cases.job(contigs, 2, 1, [(2, vcf_cases.EQ), (65535, vcf_cases.D), (2, vcf_cases.EQ)])
    lead = vcf_cases.job(contigs, 2, 1, [(65536, vcf_cases.D), (2, vcf_cases.EQ)])
    got = run(exe, "events", "\n".join([line(base, 0, contigs, d=99), line(base, 0, contigs, use=0, strand=0), line(ok, 0, contigs), line(lead, 0, contigs)]) + "\n", 4)
    want = [K(e) for e in vcf_ref.alleles(base, contigs)]
    assert got[0] == " ".join(f"{a}:{b}" for a, b in want) and len(want) == 3 and got[1] == "-" and got[3] == "-"
    assert got[2] == "%d:%d" % K(vcf_ref.alleles(ok, contigs)[0]) and vcf_ref.alleles(ok, contigs)[0][2:] == ("D", 65535) and big["runs"][1] >> 4 == 65536


@pytest.mark.parametrize("world", vcf_cases.finish_worlds(), ids=lambda w: w[0])
def test_finish(exe, world):
    name, contigs, t, iv, min_count, min_frac = world
    want = vcf_ref.finish(t, iv, contigs, min_count, min_frac)
    text = (f"{min_count} {min_frac!r} {len(contigs)} {len(t)} {len(iv)}\n" + "".join("=" + c.decode("latin-1") + "\n" for c in contigs)
            + "".join(f"{k[0]} {k[1]} {t[k]}\n" for k in sorted(t)) + "".join(f"{c} {a} {b}\n" for c, a, b in iv))
    got = run(exe, "finish", text, len(want))
    assert got == [f"A {a} {b} {n} {d} {w.hex()}" for a, b, n, d, w in want]
    if name == "edges":                                            # the restatement itself, by hand
        assert [(n, d) for _, _, n, d, _ in want] == [(2, 2), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (2, 2), (2, 2), (1, 1), (1, 1), (2, 2), (2, 2), (1, 2), (2, 2), (2, 2)]
        assert [len(w.rstrip(b"\0")) for _, _, _, _, w in want] == [25, 25, 25, 25, 25, 25, 25, 24, 1, 25, 25, 25, 24, 24, 2, 1]
    if name == "count_eq_min_count":
        assert [n for _, _, n, _, _ in want] == [2] * 8
    if name == "frac_half":
        assert [(n, d) for _, _, n, d, _ in want] == [(2, 4), (2, 4), (2, 3)]
