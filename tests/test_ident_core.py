"""The definition of the identity filter and the checks on mm_ident_filter's arguments (metamaps_amd/csrc/mm_ident_core.hpp), built for the host with g++ —
plain, and as a stand-alone program under the address and undefined-behaviour sanitizers — against the naive restatement (tests/ident_ref.py): the edge
cases, 200 random problems, and the 73 reads of tests/golden/example/example.EM.  CPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ident_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def unbits(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("ident") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_ident_core.cpp")], check=True, timeout=300)
    return p


def record(off, taxon, ident, best, n_taxa, thr):
    return " ".join(map(str, ["F", len(off) - 1, len(taxon), n_taxa, bits(thr)] + [int(x) for x in off] + [int(x) for x in taxon] + [bits(x) for x in ident] + [int(x) for x in best]))


def ask(exe, problems):
    p = subprocess.run([exe], input=("\n".join(record(*q) for q in problems) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = []
    for line in p.stdout.decode().splitlines():
        if line.startswith("refused"):
            out.append(int(line.split()[1]))
            continue
        part = [x.split() for x in line.split(";")[:-1]]
        ints = lambda k: np.array([int(x) for x in part[k]], dtype=np.int64)
        dbl = lambda k: np.array([unbits(x) for x in part[k]], dtype=np.float64)
        out.append(dict(sorted_max=dbl(0), n_le=int(part[1][0]), taxon_reads=ints(2), taxon_median=dbl(3), taxon_removed=ints(4).astype(bool),
                        read_removed=ints(5).astype(bool), read_src=ints(6), entry_src=ints(7), read_off_out=ints(8)))
    assert len(out) == len(problems)
    return out


def check(exe, problems):
    got = ask(exe, problems)
    for k, (g, q) in enumerate(zip(got, problems)):
        assert isinstance(g, dict), (k, g)
        ident_ref.same(g, ident_ref.filter_arrays(*q))
    return got


def one_entry_reads(taxon, ident):
    n = len(taxon)
    return (np.arange(n + 1), taxon, ident, np.arange(n))


def random_problem(rng, k):
    nr = int(rng.integers(0, 40))
    sizes = rng.choice([0, 1, 1, 2, 3, 17, 70], size=nr)
    if k % 40 == 0:
        sizes[:] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ne = int(off[-1])
    n_taxa = int(rng.integers(1, 8))
    taxon = rng.integers(0, n_taxa, size=ne)
    pool = rng.integers(0, 9, size=ne) / 8.0 * 100 if k % 2 else rng.integers(7000, 10001, size=ne) / 100.0      # eighths: many ties
    ident = rng.choice(pool.tolist() + [0.0, 100.0], size=ne)
    best = np.array([int(rng.integers(off[r], off[r + 1])) if off[r + 1] > off[r] else int(rng.integers(-3, 3)) for r in range(nr)], dtype=np.int64)
    thr = float(rng.choice([0.0, 50.0, 62.5, 85.0, 87.5, 100.0, 101.0, float(rng.integers(7000, 10001)) / 100.0]))
    return off, taxon, ident, best, n_taxa, thr


def test_edges(exe):
    e = np.zeros(0)
    sizes = [1, 2, 3, 4, 5]                                         # ranks 0, 1, 1, 2, 2 of the ascending identities
    tx = np.repeat(np.arange(5), sizes)
    idn = np.concatenate([10.0 * t + np.arange(n)[::-1] for t, n in enumerate(sizes)])
    problems = [([0], e, e, e, 3, 80.0),                            # zero reads
                ([0, 0, 0, 0], e, e, [0, 5, -1], 3, 80.0),          # only empty reads (their best is ignored)
                ([0, 1], [0], [85.5], [0], 1, 80.0),                # one read with one entry
                one_entry_reads(tx, idn) + (6, 25.0),               # taxon 5 has no read: NaN, not removed
                one_entry_reads([0, 0, 0, 1, 1, 1], [70, 80, 90, 70, np.nextafter(80.0, 0), 90]) + (2, 80.0),   # a median equal to thr stays, the double below it goes
                one_entry_reads([0, 1, 0, 1], [77.5, 77.5, 77.5, 77.5]) + (2, 77.5),       # all identities equal
                ([0, 2, 4], [0, 1, 1, 0], [99.0, 60.0, 50.0, 95.0], [1, 2], 2, 80.0),    # the largest identity is not the best entry's
                one_entry_reads([0, 1, 2], [10.0, 50.0, 99.0]) + (3, 0.0),                 # thr 0 removes nothing
                one_entry_reads([0, 1, 2], [10.0, 50.0, 99.0]) + (3, 100.0),               # thr 100 and thr above 100 remove everything
                one_entry_reads([0, 1, 2], [10.0, 50.0, 99.0]) + (3, 150.0),
                one_entry_reads([0, 0, 0], [0.0, -0.0, 0.0]) + (1, 0.0)]                   # -0.0 is 0
    got = check(exe, problems)
    assert got[0]["read_off_out"].tolist() == [0] and got[1]["read_off_out"].tolist() == [0] and len(got[1]["sorted_max"]) == 0
    assert got[3]["taxon_median"][:5].tolist() == [0.0, 11.0, 21.0, 32.0, 42.0] and np.isnan(got[3]["taxon_median"][5]) and not got[3]["taxon_removed"][5]
    assert got[3]["taxon_removed"].tolist() == [True, True, True, False, False, False]
    assert got[4]["taxon_removed"].tolist() == [False, True]
    assert not got[5]["taxon_removed"].any() and got[5]["n_le"] == 4
    assert got[6]["sorted_max"].tolist() == [95.0, 99.0]
    assert got[6]["taxon_reads"].tolist() == [0, 2] and got[6]["taxon_median"][1] == 60.0 and got[6]["entry_src"].tolist() == [0, 3]   # both reads lose their best, keep one entry
    assert not got[7]["taxon_removed"].any() and got[7]["n_le"] == 0
    for g in got[8:10]:
        assert g["taxon_removed"].all() and len(g["read_src"]) == 0 and g["read_off_out"].tolist() == [0]
    assert bits(got[10]["sorted_max"][0]) == 0 and bits(got[10]["taxon_median"][0]) == 0


def test_200_random_problems(exe):
    rng = np.random.default_rng(51)
    problems = [random_problem(rng, k) for k in range(200)]
    got = check(exe, problems)
    assert sum(1 for g in got if g["taxon_removed"].any() and not g["taxon_removed"].all()) > 50
    assert sum(1 for g, q in zip(got, problems) if 0 < len(g["read_src"]) < np.count_nonzero(np.diff(q[0]))) > 20      # reads that lose every entry


def test_refusals(exe):
    ok = ([0, 2, 3], [0, 1, 1], [90.0, 80.0, 70.0], [1, 2], 2, 80.0)
    change = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
    cases = [(ok, None), (change(0, [1, 2, 3]), 2), (change(0, [0, 3, 2]), 2), (change(1, [0, 2, 1]), 3), (change(1, [0, -1, 1]), 3),
             (change(3, [2, 2]), 4), (change(3, [0, 1]), 4), (change(3, [-1, 2]), 4), (change(2, [90.0, -0.5, 70.0]), 5), (change(2, [90.0, float("nan"), 70.0]), 5),
             (change(5, float("nan")), 6), (change(2, [90.0, -0.0, float("inf")]), None), (change(5, float("inf")), None), (change(5, -1.0), None)]
    got = ask(exe, [c for c, _ in cases])
    for g, (_, code) in zip(got, cases):
        assert (g == code) if code else isinstance(g, dict), (g, code)


def example_problem():
    """the 73 reads of the reference's example output: taxon from the contig ID, identity from field 12, best = the first line with the highest last field"""
    reads = ident_ref.read_groups(os.path.join(HERE, "golden", "example", "example.EM"))
    ids = sorted({ident_ref.TAXID.search(f[5]).group(1) for g in reads for f in g})
    off = np.concatenate([[0], np.cumsum([len(g) for g in reads])])
    taxon = [ids.index(ident_ref.TAXID.search(f[5]).group(1)) for g in reads for f in g]
    ident = [float(f[12]) for g in reads for f in g]
    best = [int(off[r]) + max(range(len(g)), key=lambda k: (float(g[k][13]), -k)) for r, g in enumerate(reads)]
    return reads, ids, (off, taxon, ident, best, len(ids))


def test_reference_example_medians(exe):
    reads, ids, p = example_problem()
    assert len(reads) == 73 and p[2][0] == 85.5956
    got = check(exe, [p + (80.0,), p + (86.0,)])
    assert got[0]["taxon_reads"].sum() == 73 and len(got[0]["sorted_max"]) == 73
    assert 0 < got[1]["taxon_removed"].sum() < np.count_nonzero(got[1]["taxon_reads"])
