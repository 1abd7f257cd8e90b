"""The LCA assignment's core (metamaps_amd/csrc/mm_lca_core.hpp), built for the host with g++ — plain, and with the address and undefined-
behaviour sanitizers — against a brute-force Python restatement of its definition ("LCA assignment"; tests/lca_ref.py):
for every node the posteriors below it are summed by walking parents, the deepest qualifying node is the answer.  Posteriors are multiples
of 2^-20 that sum to 1, so every mass is exact and node and mass must match exactly, also where a mass equals the threshold."""
import os
import struct
import subprocess

import numpy as np
import pytest

import lca_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXED_TAUS = (0.51, 0.75, 0.8, 1.0)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def unbits(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lca") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_lca_core.cpp")], check=True, timeout=300)
    return p


def ask(exe, text):
    p = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout.decode().splitlines()


def trees():
    rng = np.random.default_rng(20)
    out = [("root", np.zeros(1, dtype=np.int32)), ("chain40", lca_ref.random_tree(rng, 41, "chain")), ("star", lca_ref.random_tree(rng, 300, "star")),
           ("pair", np.zeros(3, dtype=np.int32))]
    for k in range(10):
        out.append((f"random{k}", lca_ref.random_tree(rng, int(rng.integers(2, 301)), "random")))
        out.append((f"deep{k}", lca_ref.random_tree(rng, int(rng.integers(2, 301)), "deep")))
    return out


def reads_for(rng, parent, n_reads):
    """entries on leaves AND internal nodes: any node of the tree, or any node below a random one (a deep LCA)"""
    n = len(parent)
    out = []
    for i in range(n_reads):
        k = int(rng.choice([1, 2, 3, 5, 17, 64, 65, 300])) if i % 3 else int(rng.integers(1, 301))
        if rng.random() < 0.5 and n > 1:
            top = int(rng.integers(0, n))
            below = [v for v in range(n) if _has_ancestor(parent, v, top)]
            nodes = rng.choice(below, size=k)
        else:
            nodes = rng.integers(0, n, size=k)
        out.append((nodes.astype(np.int32), lca_ref.exact_posteriors(rng, k)))
    return out


def _has_ancestor(parent, v, top):
    while v > top:
        v = parent[v]
    return v == top


def test_derivation_and_assignment_match_the_definition(exe):
    rng = np.random.default_rng(21)
    text, want, n_boundary = [], [], 0
    for name, parent in trees():
        depth = lca_ref.depths(parent)
        text.append(f"T {len(parent)} " + " ".join(map(str, parent.tolist())))
        want.append(("tree", name, parent, depth))
        for nodes, p in reads_for(rng, parent, 24):
            _, _, masses = lca_ref.brute_one(parent, depth, nodes, p, 0.51)
            chain = [m for m in masses.values() if m >= 0.51]       # the exact mass of a node on the read's chain: a mass EQUAL to the threshold
            taus = list(FIXED_TAUS)
            if chain:
                taus.append(max(0.51, float(rng.choice(chain))))
                n_boundary += 1
            for tau in taus:
                text.append(f"R {bits(tau)} {len(nodes)} " + " ".join(f"{v} {bits(x)}" for v, x in zip(nodes.tolist(), p.tolist())))
                want.append(("read", name, lca_ref.brute_one(parent, depth, nodes, p, tau)[:2], tau))
    assert n_boundary > 400
    got = iter(ask(exe, "\n".join(text) + "\n"))
    for w in want:
        if w[0] == "tree":
            _, name, parent, depth = w
            assert next(got) == "tree 1", name
            d, tin, tout = (np.array(next(got).split(), dtype=np.int64) for _ in range(3))
            assert np.array_equal(d, depth), name
            assert sorted(tin.tolist()) == list(range(len(parent))), name          # a numbering of the nodes
            for v in range(len(parent)):                                          # a in the subtree of v  <=>  tin[v] <= tin[a] < tout[v]
                inside = np.array([_has_ancestor(parent, a, v) for a in range(len(parent))])
                assert np.array_equal(inside, (tin >= tin[v]) & (tin < tout[v])), (name, v)
        else:
            _, name, (node, mass), tau = w
            g = next(got).split()
            assert (int(g[0]), unbits(g[1])) == (node, mass), (name, tau, g)


def test_vectorised_reference_agrees_with_the_definition():
    """tests/lca_ref.assign (what the GPU tests compare against) against brute_one"""
    rng = np.random.default_rng(22)
    for name, parent in trees()[:12]:
        depth = lca_ref.depths(parent)
        reads = reads_for(rng, parent, 12)
        off = np.concatenate([[0], np.cumsum([len(n) for n, _ in reads])])
        for tau in FIXED_TAUS:
            lca, mass, direct, _ = lca_ref.assign(parent, off, np.concatenate([n for n, _ in reads]), np.concatenate([p for _, p in reads]), tau)
            for r, (nodes, p) in enumerate(reads):
                assert (int(lca[r]), float(mass[r])) == lca_ref.brute_one(parent, depth, nodes, p, tau)[:2], (name, tau, r)
            assert np.array_equal(direct, np.bincount(lca, minlength=len(parent)))


def test_bad_trees_taxa_and_thresholds_are_refused(exe):
    bad_trees = ["T 0", "T 1 1", "T 3 0 1 1", "T 3 0 2 0", "T 3 0 0 -1", "T 2 1 0", "T 3 0 0 3"]
    out = ask(exe, "\n".join(bad_trees) + "\n")
    assert out == ["tree 0"] * len(bad_trees)
    taus = [(0.51, 1), (1.0, 1), (0.75, 1), (0.5, 0), (0.5099999, 0), (np.nextafter(1.0, 2.0), 0), (0.0, 0), (-1.0, 0), (2.0, 0), (float("nan"), 0), (float("inf"), 0)]
    out = ask(exe, "\n".join(f"H {bits(t)}" for t, _ in taus) + "\n")
    assert out == [f"thr {ok}" for _, ok in taus]
    out = ask(exe, "X 3 4 0 1 2 2\nX 3 2 0 3\nX 3 2 -1 0\nX 1 1 0\n")
    assert out == ["taxa 1", "taxa 0", "taxa 0", "taxa 1"]
