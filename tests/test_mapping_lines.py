"""The device-free half of `classify` (metamaps_amd/csrc/host/mapping_lines.hpp, classify_tables.hpp, clean_frequencies of taxonomy.hpp): the tokeniser that cuts
a mappings file into pieces at read boundaries, parses them on threads and joins them, adopt() for the lines mapDirectly --then-classify keeps, the per-mapping
fields with their 1/nLoc, em_shard, cleanF and the statistics of a bootstrap row.  tests/test_mapping_lines.cpp includes the two headers alone, is built with g++
plain, under the address and undefined-behaviour sanitizers and under the thread sanitizer, and run as a stand-alone program.  The expected values of off, taxon,
mapq and 1/nLoc are those of metamaps_amd/emhost.py::load_problem, an independent restatement; the other fields come from str.split.  Every comparison of a parsed
value is exact: both sides parse the same decimal text, and 1/nLoc is one division.  CPU."""
import os
import subprocess

import numpy as np
import pytest

from metamaps_amd import emhost

HERE = os.path.dirname(os.path.abspath(__file__))
PIECES = [1, 2, 3, 7, 64]
SAN = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-O1", "-g", "-fsanitize=thread"]}


@pytest.fixture(scope="module", params=list(SAN))
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("mapping_lines_" + request.param) / "t")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", *SAN[request.param], "-o", p, os.path.join(HERE, "test_mapping_lines.cpp"), "-lpthread"],
                   check=True, timeout=600)
    return p


# taxon 5: three contigs of 3000, 800 and 120 bases; taxon x7: one of 1500; taxon 9: one of 50.  C_ABSENT carries taxon 5 and is not in taxonInfo.txt.
TAXON_INFO = {"5": {"kraken:taxid|5|C1": 3000, "kraken:taxid|5|C2": 800, "kraken:taxid|5|C3": 120}, "x7": {"kraken:taxid|x7|D1": 1500}, "9": {"kraken:taxid|9|LATE": 50}}
ABSENT = "kraken:taxid|5|C_ABSENT"
MAPQS = ["1", "0.5", "1e-05", "1e-320", "0.333333", "2.5e-11"]


def line(rid, rlen, contig, k, mapq):
    start = 10 + 3 * k
    return f"{rid} {rlen} 0 {rlen - 1} + {contig} {TAXON_INFO.get(contig.split('|')[1], {}).get(contig, 999)} {start} {start + rlen - 1} {87.5 + (k % 9) / 8} 20 25 {91.25 + k % 5} {mapq}"


def mixed_text():
    """About 300 lines in 36 reads: reads of one line and of many, one of 120 lines in the middle (every even cut into 2, 3 or 7 pieces falls inside it), IDs that
    are prefixes of their neighbours' (r1, r10, r100), read lengths on both sides of every contig length of taxon 5, the contig that taxonInfo.txt does not list,
    every shape of field 14, and a contig that only the last read maps to."""
    contigs = [c for t in ("5", "x7") for c in TAXON_INFO[t]] + [ABSENT]
    reads, k = [], 0
    lens = [100, 120, 121, 500, 800, 801, 2000, 3000, 3001, 60]
    for r in range(36):
        rid = "r1" + "0" * (r % 3) + ("" if r < 3 else f"_{r}")
        n = 120 if r == 17 else 1 if r % 4 == 0 else 2 + r % 9
        rl = lens[r % len(lens)]
        reads.append([line(rid, rl, contigs[(k + i) % len(contigs)] if r != 35 else "kraken:taxid|9|LATE", k + i, MAPQS[(k + i) % len(MAPQS)]) for i in range(n)])
        k += n
    out = []
    for r, g in enumerate(reads):
        for i, ln in enumerate(g):
            out.append(ln)
            if r == 5 and i == 1:
                out.append("")                                      # an empty line inside a read
        if r in (2, 20):
            out += ["", ""]                                         # and two between reads
    return "\n".join(out) + "\n"


def inputs():
    mixed = mixed_text()
    one_read = "\n".join(line("only", 700, c, i, MAPQS[i]) for i, c in enumerate(TAXON_INFO["5"])) + "\n"
    return {"mixed": mixed, "no_final_newline": mixed[:-1], "one_read": one_read, "one_line": line("solo", 90, ABSENT, 0, "1"), "empty": "", "only_newlines": "\n\n\n"}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The DB directory, and per input its file, its PREFIX.meta and the lines the program must print, built once."""
    d = tmp_path_factory.mktemp("mapping_lines_world")
    db = str(d / "db")
    os.mkdir(db)
    with open(os.path.join(db, "taxonInfo.txt"), "w") as f:
        for t, cs in TAXON_INFO.items():
            f.write(t + " " + ";".join(f"{c}={n}" for c, n in cs.items()) + "\n")
    files, want = {}, {}
    for name, text in inputs().items():
        fn = str(d / name)
        open(fn, "w").write(text)
        open(fn + ".meta", "w").write("ReadsNotMapped 3\nReadsTooShort 2\nTotalReads 99\nReadsMapped 94\n")
        files[name] = fn
        want[name] = expected(fn, db, text)
    return {"db": db, "files": files, "want": want}


def expected(fn, db, text):
    rows = [ln for ln in text.split("\n") if ln]
    contigs = list(dict.fromkeys(ln.split(" ")[5] for ln in rows))    # first-seen order
    if not rows:
        return [("off", [0]), ("contigs", [])]
    P = emhost.load_problem(fn, db)
    out = [("off", [int(x) for x in P.read_off]), ("contigs", contigs), ("taxa", list(P.taxa))]
    assert [ln for g in P.lines for ln in g] == rows
    for i, ln in enumerate(rows):
        f = ln.split(" ")
        out.append(("L", f[0], len(ln), ln.rindex(" "), f[5], int(f[1]), int(f[7]), int(f[8]), float(f[9]) / 100.0, float(P.mapq[i]), int(P.taxon[i]), float(P.inv_nloc[i])))
    return out


def parsed(stdout):
    out = []
    for ln in stdout.decode().splitlines():
        f = ln.split(" ")
        if f[0] == "off":
            out.append(("off", [int(x) for x in f[1:]]))
        elif f[0] in ("contigs", "taxa"):
            out.append((f[0], f[1:]))
        else:
            assert f[0] == "L" and len(f) == 12, ln
            out.append(("L", f[1], int(f[2]), int(f[3]), f[4], int(f[5]), int(f[6]), int(f[7]), float(f[8]), float(f[9]), int(f[10]), float(f[11])))
    return out


def run(exe, *args, rc=0):
    p = subprocess.run([exe, *args], capture_output=True, timeout=120)
    assert p.returncode == rc, (p.stdout + p.stderr).decode()[-3000:]
    return p


@pytest.mark.parametrize("name", list(inputs()))
def test_tokenise_and_fields_in_every_piece_count(exe, world, name):
    outs = [run(exe, "parse", world["files"][name], world["db"], str(n)).stdout for n in PIECES]
    assert all(o == outs[0] for o in outs), [PIECES[i] for i, o in enumerate(outs) if o != outs[0]]
    assert parsed(outs[0]) == world["want"][name]                  # exact: ==, also on the doubles


def test_the_inputs_hold_the_cases_they_are_meant_to(world):
    """The +1 term of nLoc on both sides and for the unlisted contig, the denormal as 0, a read across every even cut, fewer reads than 64, the late contig."""
    want = world["want"]["mixed"]
    rows = [w for w in want if w[0] == "L"]
    off = want[0][1]
    assert len(off) - 1 == 36 and 250 < len(rows) < 400
    assert max(b - a for a, b in zip(off, off[1:])) == 120 and min(b - a for a, b in zip(off, off[1:])) == 1
    text = inputs()["mixed"]
    big = text.index("\nr100_17 ") + 1                             # the 120-line read: from the start of its second line to its end
    lo, hi = text.index("\n", big) + 1, text.index("\nr1_18 ")
    for n in (2, 3, 7):                                            # an even cut into 2, 3 and 7 pieces falls inside it
        assert any(lo < len(text) // n * t < hi for t in range(1, n)), n
    assert want[1][1][-1] == "kraken:taxid|9|LATE" and want[2][1] == ["5", "9", "x7"]
    assert any(r[9] == 0.0 for r in rows) and {1.0, 0.5, 1e-05} <= {r[9] for r in rows}
    # taxon 5 for a read of 801 bases with mappings on C1, C2, C3: 3000 - 801 + 1 on C1, + 1 for each of C2 and C3 it hits; the unlisted contig adds nothing
    r801 = [r for r in rows if r[5] == 801 and r[10] == 0]
    assert r801 and {r[11] for r in r801} <= {1.0 / (2200 + k) for k in (0, 1, 2)}
    longer = lambda L: sum(n - L + 1 for n in TAXON_INFO["5"].values() if n >= L)    # the contigs at least as long as the read
    assert {0, 1, 2} <= {round(1 / r[11]) - longer(r[5]) for r in rows if r[10] == 0}   # the +1 term: absent, once and twice
    assert any(r[4] == ABSENT for r in rows)
    assert world["want"]["one_line"][-1][11] == 1.0 / (2911 + 711 + 31)   # 90 bases: every listed contig of taxon 5 is longer; the unlisted one it maps to adds nothing


@pytest.mark.parametrize("name", ["mixed", "no_final_newline", "one_read", "one_line"])
def test_adopt_gives_what_the_tokeniser_gives(exe, world, name):
    assert run(exe, "adopt", world["files"][name], world["db"]).stdout == run(exe, "parse", world["files"][name], world["db"], "1").stdout


REFUSALS = {
    "five_fields": ("a b c d e", "has weird format - is this a mappings file generated by MetaMap?"),
    "thirteen_fields": (" ".join(line("r", 100, ABSENT, 0, "1").split(" ")[:13]), "has lines with fewer than 14 fields - is this a mappings file generated by MetaMap?"),
    "not_a_number": (line("r", 100, ABSENT, 0, "high"), "has a mapping quality that is not a number"),
    "overflow": (line("r", 100, ABSENT, 0, "1e999"), "mapping quality out of range in "),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(exe, world, tmp_path, name):
    bad, msg = REFUSALS[name]
    fn = str(tmp_path / "bad")
    good = line("q", 100, ABSENT, 1, "1")
    open(fn, "w").write(good + "\n" + bad + "\n" + good + "\n")
    for n in ("1", "3"):
        p = run(exe, "parse", fn, world["db"], n, rc=1)
        assert msg in p.stderr.decode() and fn in p.stderr.decode() and p.stdout == b""


def test_em_shards_tile_the_reads(exe):
    rows = [[int(x) for x in ln.split()] for ln in run(exe, "shards").stdout.decode().splitlines()]
    assert len(rows) == 3 * (1 + 2 + 3 + 8)
    for NR in (0, 1, 5):
        for G in (1, 2, 3, 8):
            sh = [r for r in rows if r[0] == NR and r[1] == G]
            assert [r[2] for r in sh] == list(range(G))
            assert sh[0][3] == 0 and sh[-1][4] == NR and all(a[4] == b[3] for a, b in zip(sh, sh[1:]))   # [lo, hi) in order, end to start
            sizes = [r[4] - r[3] for r in sh]
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            for r in sh:
                assert r[6] == 0 and len(r[6:]) == r[4] - r[3] + 1                  # soff rebased to 0, one entry per read and the end
            assert sum(r[-1] for r in sh) == sum(1 + (i * 7 % 4) for i in range(NR))   # every mapping in exactly one shard


def test_clean_frequencies_by_hand(exe):
    def clean(n, *items):
        return {kv.split("=")[0]: float(kv.split("=")[1]) for kv in run(exe, "clean", str(n), *items).stdout.decode().split()}
    # 10 mapped reads: the floor is 0.09.  b lies below it without a read and goes; c lies below it with a read and stays; the rest sums to 0.95
    got = clean(10, "a=0.5", "b=0.05", "c=0.05:2", "d=0.4")
    assert got == {"a": 0.5 / (0.5 + 0.05 + 0.4), "c": 0.05 / (0.5 + 0.05 + 0.4), "d": 0.4 / (0.5 + 0.05 + 0.4)}   # the sum in map order: a, c, d
    # exactly at the floor stays (the reference drops what is below it); nothing dropped: the values over their sum
    assert clean(9, "x=0.1", "y=0.9") == {"x": 0.1 / (0.1 + 0.9), "y": 0.9 / (0.1 + 0.9)}
    assert clean(4, "p=0.225", "q=0.2") == {"p": 0.225 / 0.225}    # floor 0.9 * (1 / 4) = 0.225: p stays, q goes
    assert clean(2, "m=0.25:1", "n=0.25:3") == {"m": 0.5, "n": 0.5}


@pytest.mark.parametrize("values", [[0.25, 0.75], [0.1, 0.4, 0.2, 0.5, 0.3], [0.0, 0.0, 1.0, 0.0, 0.0], [3.0, 1.0]])
def test_bootstrap_row_statistics(exe, values):
    mean, sd, lo, hi = (float(x) for x in run(exe, "stats", *[repr(v) for v in values]).stdout.split())
    assert mean == pytest.approx(sum(values) / len(values), rel=1e-15)
    assert sd == pytest.approx(np.std(values, ddof=1), rel=1e-12)
    assert lo == pytest.approx(np.quantile(values, 0.025), rel=1e-14, abs=1e-300) and hi == pytest.approx(np.quantile(values, 0.975), rel=1e-14)
    if values == [0.25, 0.75]:                                     # by hand: SD over n - 1 = sqrt(2 * 0.25^2), the quantiles 2.5 % in from the two values
        assert (mean, lo, hi) == (0.5, 0.25 + 0.025 * 0.5, 0.25 + 0.975 * 0.5) and sd == pytest.approx(0.5 ** 0.5 / 2, rel=1e-15)
