"""The device-free host code of mapDirectly --extract-* (metamaps_amd/csrc/host/reads_out.hpp: the options, the list grammar, the primary line and which reads
each file takes; the rows of side_files.hpp), compiled on its own with g++ under the address and undefined-behaviour sanitizers and run as a stand-alone
program (tests/test_reads_out_host.cpp), against tests/reads_out_ref.py.  CPU."""
import os
import random
import subprocess

import pytest

import reads_out_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CONTIGS = ["c0|kraken:taxid|10000|a", "c1|kraken:taxid|x7001|b", "c2|kraken:taxid|10000|c", "c3|kraken:taxid|77|kraken:taxid|10000"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("reads_out_host") / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", p, os.path.join(HERE, "test_reads_out_host.cpp"), "-lpthread", "-lz"], check=True, timeout=600)
    return p


def _opts(exe, *args):
    p = subprocess.run([exe, "opts", *args], capture_output=True, timeout=60)
    return p.returncode, (p.stdout + p.stderr).decode().strip()


def test_the_list_grammar(exe):
    assert _opts(exe) == (0, "0 0 0 0 | 0 | |")
    assert _opts(exe, "extract-unmapped", "base-qualities") == (0, "1 0 0 0 | 1 | |")
    assert _opts(exe, "extract-mapped", "pileup", "min-base-quality=10") == (0, "0 1 0 0 | 1 | |")   # (it implies --base-qualities: FASTQ records and .fq.gz)
    assert _opts(exe, "extract-mapped", "extract-taxa=10000,x7001,0", "deplete-taxa=x1") == (0, "0 1 1 1 | 0 | 10000 x7001 0 | x1")
    many = ",".join(str(i) for i in range(64))
    assert _opts(exe, f"deplete-taxa={many}")[0] == 0
    for flag in ("extract-taxa", "deplete-taxa"):
        for bad in ("", ",", "10000,", ",10000", "10000,,x7001", "abc", "x", "12x", "xx1", "X1", "-1", "1.5", " 1", "x7001,x7001", "1,2,1", many + ",64"):
            rc, said = _opts(exe, f"{flag}={bad}")
            assert rc == 1 and f"--{flag}" in said, (flag, bad, said)
    rc, said = _opts(exe, "extract-taxa=5", "deplete-taxa=5,5")    # each list is its own
    assert rc == 1 and "--deplete-taxa" in said and "twice" in said


def test_suffixes_and_what_the_rows_imply(exe):
    p = subprocess.run([exe, "suffix"], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode().splitlines() == ["extract-unmapped .unmapped.fq.gz .unmapped.fa.gz", "extract-mapped .mapped.fq.gz .mapped.fa.gz",
                                               "extract-taxa .taxa.fq.gz .taxa.fa.gz", "deplete-taxa .depleted.fq.gz .depleted.fa.gz",
                                               "0 1 1 1 0"]          # (--paf implies --edit-distance; a read file does not)


def _select(exe, args, off, lines):
    text = " ".join(CONTIGS) + "\n" + " ".join(map(str, off)) + "\n" + "".join(f"{c} {q}\n" for c, q in lines)
    p = subprocess.run([exe, "select", *args], input=text.encode(), capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode().splitlines()
    return [int(x) for x in out[0].split()], {ln.split(":")[0]: [int(x) for x in ln.split(":")[1].split()] for ln in out[1:]}


def _ref_lines(off, lines):
    """the same world as lines of a PREFIX: field 1 the read, field 6 the contig, field 14 the printed value"""
    out = []
    for r in range(len(off) - 1):
        for c, q in lines[off[r]:off[r + 1]]:
            out.append(" ".join([f"r{r}", "0", "0", "0", "+", CONTIGS[c]] + ["0"] * 7 + [q]))
    return out


def test_the_primary_line_and_the_four_selections(exe):
    # read 0: two equal field-14 values, the first wins (contig 1, the listed taxon); read 1: no line (too short or not mapped); read 2: the larger value is
    # second; read 3: equal values, the first is on an unlisted contig; read 4: the first key of a contig name with two decides (77, not 10000)
    off = [0, 2, 2, 4, 6, 7]
    lines = [(1, "0.5"), (0, "0.5"), (0, "0.2"), (1, "0.90"), (2, "1"), (1, "1"), (3, "0.3")]
    args = ["extract-unmapped", "extract-mapped", "extract-taxa=x7001,77", "deplete-taxa=x7001"]
    primary, sel = _select(exe, args, off, lines)
    assert primary == [1, -1, 1, 2, 3]
    assert sel == {"unmapped": [1], "mapped": [0, 2, 3, 4], "taxa": [0, 2, 4], "depleted": [1, 3, 4]}
    ids = [f"r{r}" for r in range(5)]
    want = ref.selections(_ref_lines(off, lines), ids, {"x7001", "77"})
    assert sel["taxa"] == want["taxa"] and sel["mapped"] == want["mapped"] and sel["unmapped"] == want["unmapped"]
    assert sel["depleted"] == ref.selections(_ref_lines(off, lines), ids, {"x7001"})["depleted"]
    # a too-short read under --deplete-taxa alone is kept; an x-prefixed ID is not its number
    primary, sel = _select(exe, ["deplete-taxa=7001"], off, lines)
    assert sel == {"depleted": [0, 1, 2, 3, 4]}
    primary, sel = _select(exe, ["deplete-taxa=x7001,10000,77"], off, lines)
    assert sel == {"depleted": [1]}


def test_random_worlds_against_the_restatement(exe):
    rng = random.Random(4)
    for _ in range(40):
        n = rng.randrange(1, 12)
        off = [0]
        for _ in range(n):
            off.append(off[-1] + rng.choice([0, 0, 1, 1, 2, 3]))
        lines = [(rng.randrange(4), rng.choice(["0", "1", "0.5", "0.25", "1e-05", "0.999999"])) for _ in range(off[-1])]
        taxa = rng.sample(["10000", "x7001", "77", "5"], rng.randrange(1, 4))
        _, sel = _select(exe, ["extract-unmapped", "extract-mapped", "extract-taxa=" + ",".join(taxa), "deplete-taxa=" + ",".join(taxa)], off, lines)
        assert sel == ref.selections(_ref_lines(off, lines), [f"r{r}" for r in range(n)], set(taxa))


def test_a_contig_without_a_taxon_ends_the_run(exe):
    text = "c0|kraken:taxid|1 plain_contig\n0 0\n"
    p = subprocess.run([exe, "select", "extract-taxa=1"], input=text.encode(), capture_output=True, timeout=60)
    assert p.returncode == 1 and "Could not extract taxon ID from contig identifier 'plain_contig'" in (p.stdout + p.stderr).decode()
    p = subprocess.run([exe, "select", "extract-mapped"], input=text.encode(), capture_output=True, timeout=60)   # (no taxon flag: the names are not looked at)
    assert p.returncode == 0


def test_the_reference_headers_are_scanned_before_any_device_work(exe, tmp_path):
    import gzip
    good = b">c0|kraken:taxid|10000 a comment\n" + b"ACGT" * 30000 + b"\nAC>GT\n>c1|kraken:taxid|x7\nAC\n"    # a line longer than the scan's buffer; '>' inside a line
    bad = good + b">plain_contig kraken:taxid|5 in the comment only\nACGT\n"
    for name, data, opener in (("g.fa", good, open), ("g.fa.gz", good, gzip.open), ("b.fa", bad, open), ("b.fa.gz", bad, gzip.open)):
        with opener(tmp_path / name, "wb") as f:
            f.write(data)
    for name in ("g.fa", "g.fa.gz"):
        p = subprocess.run([exe, "scan", str(tmp_path / name), "deplete-taxa=1"], capture_output=True, timeout=60)
        assert p.returncode == 0 and p.stdout.decode().strip() == "ok", p.stderr.decode()
    for name in ("b.fa", "b.fa.gz"):
        p = subprocess.run([exe, "scan", str(tmp_path / name), "extract-taxa=1"], capture_output=True, timeout=60)
        assert p.returncode == 1 and "Could not extract taxon ID from contig identifier 'plain_contig'" in (p.stdout + p.stderr).decode()
        p = subprocess.run([exe, "scan", str(tmp_path / name), "extract-mapped"], capture_output=True, timeout=60)    # (no taxon flag: no scan)
        assert p.returncode == 0
