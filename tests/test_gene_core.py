"""The stabbing query of the gene-level analysis and the checks on mm_gene_overlap's arguments (metamaps_amd/csrc/mm_gene_core.hpp), built for the host
with g++ — plain, and as a stand-alone program under the address and undefined-behaviour sanitizers — against all-pairs overlap (tests/gene_ref.py) on
2 000 random instances; and gene_ref's vectorised restatement (what the GPU tests compare against) against its plain loops.  CPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gene_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gene") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_gene_core.cpp")], check=True, timeout=300)
    return p


def ask(exe, text):
    p = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout.decode().splitlines()


def instance(rng, k):
    """a few contigs (some without genes) of short length, so that equal Starts, equal Stops and both boundary relations are common"""
    nc = int(rng.integers(1, 5))
    L = int(rng.choice([8, 20, 60, 400]))
    per = [0 if rng.random() < 0.25 else int(rng.integers(1, 40)) for _ in range(nc)]
    if k % 50 == 0:
        per = [0] * nc                                              # no gene at all
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    gs, ge = [], []
    for n in per:
        s = np.sort(rng.integers(0, L, size=n))
        e = s + rng.integers(0, max(1, L // int(rng.choice([1, 2, 8]))), size=n)
        if n and rng.random() < 0.3:
            s[0], e[0] = 0, L + 5                                   # a gene that spans the contig
        gs.append(s); ge.append(e)
    gs = np.concatenate(gs).astype(np.int64) if gs else np.zeros(0, dtype=np.int64)
    ge = np.concatenate(ge).astype(np.int64) if ge else np.zeros(0, dtype=np.int64)
    nm = 0 if k % 37 == 0 else int(rng.integers(1, 25))
    mc = rng.integers(0, nc, size=nm)
    ms = rng.integers(0, L + 2, size=nm)
    me = ms + rng.integers(0, L, size=nm)
    for m in range(nm):                                             # the two boundary relations, on purpose: stop == a gene's Start, start == a gene's Stop
        a, b = off[mc[m]], off[mc[m] + 1]
        if b > a and rng.random() < 0.3:
            j = int(rng.integers(a, b))
            if rng.random() < 0.5:
                me[m] = gs[j]; ms[m] = max(0, me[m] - int(rng.integers(0, 5)))
            else:
                ms[m] = ge[j]; me[m] = ms[m] + int(rng.integers(0, 5))
    return off, gs, ge, mc, ms, me


def test_stab_matches_all_pairs_and_count_agrees_with_emit(exe):
    rng = np.random.default_rng(31)
    text, want, n_boundary, n_hits = [], [], 0, 0
    for k in range(2000):
        off, gs, ge, mc, ms, me = instance(rng, k)
        text.append(" ".join(map(str, ["I", len(off) - 1, len(gs), len(mc)] + off.tolist() + gs.tolist() + ge.tolist() + np.stack([mc, ms, me], axis=1).ravel().tolist())))
        pm, pg = gene_ref.all_pairs(off, gs, ge, mc, ms, me)
        want.append([sorted(pg[pm == m].tolist(), reverse=True) for m in range(len(mc))])
        for m in range(len(mc)):
            a, b = off[mc[m]], off[mc[m] + 1]
            n_boundary += int(np.any(gs[a:b] == me[m]) or np.any(ge[a:b] == ms[m]))
        n_hits += len(pm)
    assert n_boundary > 2000 and n_hits > 20000
    got = ask(exe, "\n".join(text) + "\n")
    assert len(got) == len(want)
    for k, (line, w) in enumerate(zip(got, want)):
        per = [x.split() for x in line.split(";")[:-1]]
        assert len(per) == len(w), k
        for m, (g, ww) in enumerate(zip(per, w)):
            assert int(g[0]) == int(g[1]) == len(ww), (k, m, g, ww)   # count visitor == emit visitor == all-pairs
            assert [int(x) for x in g[2:]] == ww, (k, m, g, ww)         # the genes, in descending index


def test_argument_checks(exe):
    ok_t = "T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 1 1  0 2 3  3 0 1"
    cases = [(ok_t, 0),
             ("T 0 0 0 0  0  0", 0),                                                      # nothing at all
             ("T 2 3 2 4  1 2 3  5 5 1  9 5 1  0 1 1  0 2 3  3 0 1", 1),                  # offsets do not start at 0
             ("T 2 3 2 4  0 3 2  5 5 1  9 5 1  0 1 1  0 2 3  3 0 1", 1),                  # offsets descend
             ("T 2 3 2 4  0 2 3  5 4 1  9 5 1  0 1 1  0 2 3  3 0 1", 2),                  # not sorted by Start within a contig
             ("T 2 3 2 4  0 2 3  5 5 1  9 4 1  0 1 1  0 2 3  3 0 1", 3),                  # Stop < Start
             ("T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 2 1  0 2 3  3 0 1", 4),                  # group == n_groups
             ("T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 -1 1  0 2 3  3 0 1", 4),
             ("T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 1 1  0 2 1  3", 5),                    # feature offsets descend
             ("T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 1 1  0 2 3  3 4 1", 6),                  # feature id == n_feats
             ("T 2 3 2 4  0 2 3  5 5 1  9 5 1  0 1 1  0 2 3  3 -1 1", 6)]
    assert ask(exe, "\n".join(c for c, _ in cases) + "\n") == [f"table {code}" for _, code in cases]
    maps = [(f"M 2 2  0 1 5 {bits(0.9)}  1 7 7 {bits(0.0)}", 0),
            ("M 2 0", 0),
            (f"M 2 1  2 1 5 {bits(0.9)}", 7), (f"M 2 1  -1 1 5 {bits(0.9)}", 7),
            (f"M 2 1  0 6 5 {bits(0.9)}", 8),
            (f"M 2 1  0 1 5 {bits(-0.5)}", 9), (f"M 2 1  0 1 5 {bits(float('nan'))}", 9),
            (f"M 2 1  0 1 5 {bits(float('inf'))}", 0)]
    assert ask(exe, "\n".join(c for c, _ in maps) + "\n") == [f"maps {code} {'refused' if code else 'ok'}" for _, code in maps]


def test_vectorised_reference_agrees_with_plain_loops():
    rng = np.random.default_rng(32)
    for k in range(60):
        off, gs, ge, mc, ms, me = instance(rng, k + 1)
        n_groups, n_feats = int(rng.integers(1, 12)), int(rng.integers(1, 9))
        gg = rng.integers(0, n_groups, size=len(gs))
        per = rng.integers(0, 4, size=n_groups)
        foff = np.concatenate([[0], np.cumsum(per)])
        feat = rng.integers(0, n_feats, size=int(foff[-1]))          # repeats inside a group's list included
        mi = rng.integers(0, 6, size=len(mc)) / 8.0                  # many ties
        a = gene_ref.overlap(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi)
        b = gene_ref.overlap_slow(off, gs, ge, gg, n_groups, foff, feat, n_feats, mc, ms, me, mi)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2]) and a[3] == b[3], k
