"""The BAM record encoder (metamaps_amd/csrc/mm_bam_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the address and
undefined-behaviour sanitizers — against the plain restatement of the specification (tests/bam_ref.py), byte for byte: 200 random alignments, the
built cases (tests/bam_cases.py: nibble and word edges, names that move the records across all byte residues, IUPAC and unknown read bytes on
strand -, every MD shape, the bin edges, the long-CIGAR convention at 65 535 / 65 536 / 70 000 runs) and every refusal.  CPU."""
import os
import subprocess

import pytest

import bam_cases
import bam_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("bam_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_bam_core.cpp")], check=True, timeout=300)
    return p


def line(j, k, n_sets=None, **over):
    j = dict(j, **over)
    n = k + 1 if n_sets is None else n_sets
    runs = j["runs"]
    return (f"={j['name'].decode('latin-1')} {j.get('read_index', k)} {n} {j.get('contig_index', k)} {n} {j['strand']} {j['first']} {j['d']} {j['flag']} {j['mapq']} "
            f"={j['read'].decode('latin-1')} ={j['contig'].decode('latin-1')} {len(runs)} " + " ".join(str(int(w)) for w in runs))


def run(exe, lines):
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == len(lines)
    return out


def check(exe, jobs):
    got = run(exe, [line(j, k) for k, j in enumerate(jobs)])
    for k, (g, j) in enumerate(zip(got, jobs)):
        want = bam_cases.record_of(bam_ref, j, k)
        assert g == want.hex(), (k, j["name"], len(j["read"]), j["strand"], bam_ref.decode_records(bytes.fromhex(g)) if not g.startswith("E") else g)
    return [bytes.fromhex(g) for g in got]


def test_200_random_alignments(exe):
    jobs = bam_cases.random_jobs()
    assert len(jobs) == 200 and {j["strand"] for j in jobs} == {1, -1} and min(len(j["read"]) for j in jobs) < 20 < 350 < max(len(j["read"]) for j in jobs)
    assert {w & 15 for j in jobs for w in j["runs"]} == {1, 2, 7, 8} and sum(j["d"] == 0 for j in jobs) > 5
    recs = bam_ref.decode_records(b"".join(check(exe, jobs)))
    for r, j in zip(recs, jobs):                                    # the restatement against itself: MD rebuilds the contig under the alignment
        span = sum(w >> 4 for w in j["runs"] if w & 15 != 1)
        want = "".join(c if "A" <= c <= "Z" else "N" for c in j["contig"][j["first"]:j["first"] + span].decode("latin-1").upper())
        if all(c in bam_ref.NT16 for c in want):                     # (an = base comes back as SEQ has it: a byte outside the table would read N)
            assert bam_ref.ref_from_md(r["seq"], r["cigar"], r["tags"]["MD"]) == want


def test_built_cases(exe):
    jobs = bam_cases.built_jobs()
    got = check(exe, jobs)
    starts = [sum(len(g) for g in got[:k]) for k in range(len(got))]
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    recs = {r["name"]: r for r in bam_ref.decode_records(b"".join(got))}
    assert recs[b"iupac"]["seq"] == "RCGTNYNACGT" and recs[b"iupac"]["flag"] == 0x10
    assert recs[b"exact"]["tags"]["MD"] == "300" and recs[b"eq_i_eq"]["tags"]["MD"] == "8" and recs[b"eq_i_eq"]["tag_order"] == ["NM", "MD"]
    assert recs[b"d150"]["tags"]["MD"].startswith("40^") and len(recs[b"d150"]["tags"]["MD"]) == 2 + 1 + 150 + 2
    md = recs[b"counters"]["tags"]["MD"]
    assert [int(x) for x in __import__("re").findall(r"[0-9]+", md)] == [9, 10, 99, 100, 999, 1000]
    assert recs[b"xd_dx"]["tags"]["MD"].count("^") == 2 and "0" in recs[b"xx"]["tags"]["MD"]
    md = recs[b"ref_n"]["tags"]["MD"]
    assert md.split("^")[0].endswith("N19") and "-" not in md and md.count("N") == 4 and "NR" in md
    assert [recs[n]["bin"] for n in (b"bin4681", b"bin585", b"bin73", b"bin9")] == [4681, 585, 73, 9]
    r = recs[b"runs70000"]
    assert r["cigar_field"] == [70000 << 4 | 4, 70000 << 4 | 3] and len(r["tags"]["CG"]) == 70000 and r["tag_order"] == ["NM", "MD", "CG"] and r["tags"]["NM"] == 35000
    assert len(recs[b"runs65535"]["cigar_field"]) == 65535 and "CG" not in recs[b"runs65535"]["tags"]
    assert len(recs[b"runs65536"]["cigar_field"]) == 2 and len(recs[b"runs65536"]["tags"]["CG"]) == 65536
    assert all(r["qual"] == b"\xff" * r["l_seq"] and (r["next_refID"], r["next_pos"], r["tlen"]) == (-1, -1, 0) for r in recs.values())


def test_every_rule(exe):
    cases = bam_cases.broken_jobs()
    lines = []
    for j, over, rule in cases:
        over = dict(over)
        idx = {k + "_index": over.pop(k) for k in ("read", "contig") if k in over}
        lines.append(line(dict(j, **idx), 0, 1, **over))
    assert run(exe, lines) == [f"E {rule}" for _, _, rule in cases]
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 3, 4, 5, 6, 7]


def test_a_job_that_is_not_aligned_or_has_no_bases_has_no_record(exe):
    j = bam_cases.built_jobs()[0]
    got = run(exe, [line(j, 0, d=-1, runs=[]), line(j, 0, read=b"", runs=[], d=0), line(j, 0)])
    assert got[:2] == ["-", "-"] and got[2] == bam_cases.record_of(bam_ref, j, 0).hex()
