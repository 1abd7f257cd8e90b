"""The record of mapDirectly --extract-* (metamaps_amd/csrc/mm_reads_out_core.hpp), built for the host with g++ — plain, and as a stand-alone program under
the address and undefined-behaviour sanitizers — against the plain restatement tests/reads_out_ref.py: the edge set of tests/reads_out_cases.py (every
length around the word edges, exception runs on the edges, lower case, IUPAC, qualities 0 and 93, reads without qualities, names of 1 and 254 bytes) as
FASTA and FASTQ, 200 random small sets, and every rule.  The program itself asks every byte of record_byte as well as write_record.  CPU."""
import os
import subprocess

import pytest

import reads_out_cases as cases
import reads_out_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("reads_out_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_reads_out_core.cpp")], check=True, timeout=300)
    return p


def _hex(b):
    return b.hex() if b else "."


def line(n_reads, read, with_qual, name, bases, quals):
    """bases go in as the set stores them: upper-cased"""
    return f"{n_reads} {read} {int(with_qual)} {_hex(name)} {_hex(bases.upper())} {'-' if quals is None else _hex(bytes(quals))}\n"


def run(exe, lines):
    p = subprocess.run([exe], input="".join(lines).encode(), capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = []
    for ln in p.stdout.decode().splitlines():
        w = ln.split()
        if w[0] == "R":
            out.append(int(w[1]))
        else:
            data = bytes.fromhex(w[2]) if len(w) > 2 else b""
            assert len(data) == int(w[1])
            out.append(data)
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("with_qual", [False, True])
def test_edge_set(exe, with_qual):
    reads, quals = cases.edge_reads()
    names = cases.names_for(len(reads))
    got = run(exe, [line(len(reads), i, with_qual, names[i], reads[i], quals[i]) for i in range(len(reads))])
    for i in range(len(reads)):
        assert got[i] == ref.record(names[i], reads[i], quals[i], with_qual), i
    assert sum(q is None for q in quals) > 10 and any(r != r.upper() for r in reads)


def test_the_restatement_by_hand():
    assert ref.record(b"r1", b"acgtN", [0, 93, 0xFF, 1, 2], True) == b"@r1\nACGTN\n+\n!~!\"#\n"
    assert ref.record(b"r1", b"acgtN", None, True) == b"@r1\nACGTN\n+\n!!!!!\n"
    assert ref.record(b"r1", b"acgtN", [0] * 5, False) == b">r1\nACGTN\n"
    assert ref.record(b"e", b"", None, True) == b"@e\n\n+\n\n" and ref.record(b"e", b"", None, False) == b">e\n\n"


def test_200_random_small_sets(exe):
    sets = cases.random_sets()
    assert len(sets) == 200
    lines, want = [], []
    for reads, quals, sel, names in sets:
        for wq in (False, True):
            for r, nm in zip(sel, names):
                lines.append(line(len(reads), r, wq, nm, reads[r], quals[r]))
                want.append(ref.record(nm, reads[r], quals[r], wq))
    assert len(lines) > 1000
    assert run(exe, lines) == want


def test_every_rule(exe):
    reads = [b"ACGT", b"", b"NN"]
    bad = cases.bad_records()
    assert {k for k, _, _ in bad} == {1, 2, 3}
    lines = [line(3, 0, True, b"ok", reads[0], None)] + [line(3, r, True, nm, b"", None) for _, r, nm in bad] + [line(3, 2, False, b"~", reads[2], None)]
    got = run(exe, lines)
    assert got[0] == b"@ok\nACGT\n+\n!!!!\n" and got[-1] == b">~\nNN\n"
    assert got[1:-1] == [k for k, _, _ in bad]
    for k, r, nm in bad:
        assert ref.rule(r, 3, nm) == k
    # the lowest record decides, whatever comes after it
    assert ref.refusal([0, 5, 0], 3, [b"a", b"b", b""]) == (1, 1) and ref.refusal([0, 1], 3, [b"a", b"b"]) is None
