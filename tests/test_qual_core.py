"""The quality floor of the pileup's and the VCF's walks (metamaps_amd/csrc/mm_pileup_core.hpp, mm_vcf_core.hpp) and the QUAL field of the BAM record
(mm_bam_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the address and undefined-behaviour sanitizers — against the
plain restatement tests/qual_ref.py on the built jobs of tests/qual_cases.py and on 200 random jobs.  CPU."""
import os
import subprocess

import pytest

import pileup_ref
import qual_cases
import qual_ref
import vcf_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = qual_cases.FLOOR


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("qual_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_qual_core.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def built():
    return qual_cases.built_world()


@pytest.fixture(scope="module")
def rand():
    return qual_cases.random_world()


def hexq(j):
    return "-" if j.get("qual") is None else bytes(j["qual"]).hex() or "-"


def line(j, k, contigs):
    runs = j["runs"]
    return (f"{k} {k + 1} {j['c']} {len(contigs)} {j['strand']} {j['first']} {j['d']} {j.get('use', 1)} ={j['read'].decode('latin-1')} {hexq(j)} "
            f"={contigs[j['c']].decode('latin-1')} {len(runs)} " + " ".join(str(int(w)) for w in runs))


def run(exe, args, text, n_lines):
    p = subprocess.run([exe] + args, input=text.encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == n_lines
    return out


def want_pileup(j, floor):
    e = [str(pileup_ref.key(*x)) for x in qual_ref.events(j, floor)] if pileup_ref.contributes(j) else []
    return " ".join(e) or "-"


def want_vcf(j, contigs, floor):
    e = ["%d:%d" % vcf_ref.key(x) for x in qual_ref.alleles(j, contigs, floor)] if pileup_ref.contributes(j) else []
    return " ".join(e) or "-"


def check(exe, contigs, jobs, floor, names=None):
    text = "\n".join(line(j, k, contigs) for k, j in enumerate(jobs)) + "\n"
    got_p, got_v = run(exe, ["pileup", str(floor)], text, len(jobs)), run(exe, ["vcf", str(floor)], text, len(jobs))
    for k, j in enumerate(jobs):
        assert got_p[k] == want_pileup(j, floor), ("pileup", floor, k, names[k] if names else None)
        assert got_v[k] == want_vcf(j, contigs, floor), ("vcf", floor, k, names[k] if names else None)
    return got_p, got_v


def test_restatement_by_hand(built):
    """qual_ref itself on the cases whose outcome the definition states in words"""
    contigs, jobs = built
    n = lambda name, floor=FLOOR: len(qual_ref.events(jobs[name], floor))
    assert n("x1_eq_floor") == 1 and n("x1_below") == 0 and n("x1_below", FLOOR - 1) == 1
    for size in (1, 64, 65, 200):
        for at in sorted({0, 63, 64, size - 1}):
            if at < size:
                assert n(f"x{size}_low{at}") == size - 1 and n(f"x{size}_low{at}", 0) == size
                assert n(f"i{size}_low{at}") == 0 and n(f"i{size}_low{at}", 0) == 1
        assert n(f"i{size}_high") == 1
    assert n("d_at_0_low") == 0 and n("d_at_0_kept") == 3 and n("d_at_m_low") == 0 and n("d_at_m_kept") == 3
    assert n("d_left_low") == 0 and n("d_right_low") == 0 and n("d_kept") == 4 and n("d70_left_low") == 0 and n("d70_kept") == 70
    # strand -: the low base is the first X base of the oriented read, which a forward reading of the stored bytes would keep
    rev, fwd = jobs["rev_low"], jobs["fwd_low"]
    assert [e[1] for e in qual_ref.events(rev, FLOOR)] == [60 + 9] and [e[1] for e in qual_ref.events(fwd, FLOOR)] == [60 + 9]
    assert rev["qual"] == fwd["qual"][::-1] and rev["qual"] != fwd["qual"]
    assert n("no_qual", 93) == n("no_qual", 0) == 2 + 3 + 1
    # the insertion behind 105 shifts to 99 where it is kept, and is no allele where it is dropped
    kept, dropped = qual_ref.alleles(jobs["ins_shift_kept"], contigs, FLOOR), qual_ref.alleles(jobs["ins_shift_dropped"], contigs, FLOOR)
    assert kept == [(0, 99, "I", "GG")] == vcf_ref.alleles(jobs["ins_shift_kept"], contigs) and dropped == []
    assert qual_ref.alleles(jobs["ins_shift_dropped"], contigs, 0) == kept
    for j in jobs.values():                                          # floor 0 is the walk of pileup_ref and vcf_ref
        assert qual_ref.events(j, 0) == pileup_ref.events(j) and qual_ref.alleles(j, contigs, 0) == vcf_ref.alleles(j, contigs)


@pytest.mark.parametrize("floor", [0, FLOOR, FLOOR + 1, 93])
def test_built_cases(exe, built, floor):
    contigs, jobs = built
    check(exe, contigs, list(jobs.values()), floor, list(jobs))


@pytest.mark.parametrize("floor", [0, FLOOR, 41])
def test_200_random_jobs(exe, rand, floor):
    contigs, jobs = rand
    assert len(jobs) == 200 and {j["strand"] for j in jobs} == {1, -1} and {j["c"] for j in jobs} == {0, 1}
    assert min(len(j["read"]) for j in jobs) >= 50 and max(len(j["read"]) for j in jobs) > 2500
    assert max(w >> 4 for j in jobs for w in j["runs"] if w & 15 in (1, 2, 8)) > 64
    got_p, _ = check(exe, contigs, jobs, floor)
    if floor == FLOOR:                                               # not vacuous: the floor drops a good part of the events, and not all
        all_ev = sum(len(qual_ref.events(j, 0)) for j in jobs if pileup_ref.contributes(j))
        kept = sum(len(qual_ref.events(j, floor)) for j in jobs if pileup_ref.contributes(j))
        assert 0.2 * all_ev < all_ev - kept < 0.8 * all_ev
    if floor == 41:                                                  # above every drawn quality: only the reads without qualities contribute
        assert all(g == "-" for g, j in zip(got_p, jobs) if j["qual"] is not None) and any(g != "-" for g in got_p)


def test_bam_qual(exe, built, rand):
    contigs, jobs = built
    cases = list(jobs.values()) + [j for j in rand[1] if j["d"] >= 0][:40]
    ctg = [contigs[j["c"]] for j in jobs.values()] + [rand[0][j["c"]] for j in cases[len(jobs):]]
    text = "".join(f"{j['strand']} {j['first']} ={j['read'].decode('latin-1')} {hexq(j)} ={c.decode('latin-1')} {len(j['runs'])} " + " ".join(str(int(w)) for w in j["runs"]) + "\n"
                   for j, c in zip(cases, ctg))
    got = run(exe, ["qual"], text, len(cases))
    for g, j in zip(got, cases):
        assert g == qual_ref.bam_qual(j).hex() + " same"
    assert any(j["qual"] is None for j in cases) and {j["strand"] for j in cases if j["qual"] is not None} == {1, -1}
