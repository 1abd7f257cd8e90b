"""`classify --lca T` and `mapDirectly --then-classify --lca T`: PREFIX.EM.reads2Taxon.lca and PREFIX.EM.kreport beside unchanged outputs, both
recomputed in Python from PREFIX.EM, the taxonomy and .meta (tests/lca_ref.py), the invariants of a Kraken report, and the refusals of the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import lca_ref
from test_gpu_cli import CLI
from test_gpu_cli_bootstrap import OUTS, _copy_mappings

pytestmark = pytest.mark.gpu
NEW = (".EM.reads2Taxon.lca", ".EM.kreport")
CODES = {"superkingdom": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G", "species": "S"}


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=900)


def _classify(run, tag, extra):
    dst = str(run["dir"] / tag)
    _copy_mappings(run["m"], dst)
    p = _run(["classify", "--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"] + extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dst


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("lca")
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7)      # strain pairs 3 % apart: many reads split between two strains
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=1000, read_len=3000, seed=3)
    out = {"dir": d, "db": db, "q": rd["path"], "m": str(d / "map0")}
    p = _run(["mapDirectly", "--all", "-r", db.fasta, "-q", rd["path"], "-o", out["m"]])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out["plain"] = _classify(out, "plain", [])
    out["lca"] = _classify(out, "lca08", ["--lca", "0.8"])
    return out


def _same_old_outputs(a, b):
    for suf in OUTS:
        assert os.path.exists(a + suf) == os.path.exists(b + suf), suf
        if os.path.exists(a + suf):
            assert open(a + suf, "rb").read() == open(b + suf, "rb").read(), suf
    assert os.path.exists(a + ".EM") and os.path.exists(a + ".EM.WIMP")


def test_old_outputs_unchanged_and_no_new_file_without_the_flag(run):
    _same_old_outputs(run["plain"], run["lca"])
    for suf in NEW:
        assert not os.path.exists(run["plain"] + suf) and os.path.getsize(run["lca"] + suf) > 0, suf


def test_then_classify_writes_the_same_files(run):
    o = str(run["dir"] / "direct")
    p = _run(["mapDirectly", "--all", "-r", run["db"].fasta, "-q", run["q"], "-o", o, "--then-classify", run["db"].dir, "--minreads", "3", "--lca", "0.8"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _same_old_outputs(run["plain"], o)
    for suf in NEW:
        assert open(o + suf, "rb").read() == open(run["lca"] + suf, "rb").read(), suf


def test_two_logical_devices_write_the_same_files(run):
    two = _classify(run, "two", ["--lca", "0.8", "--devices", "0,0", "--em-host-reduce"])   # each rank assigns its half of the reads, the direct counts are added
    for suf in NEW:
        assert open(two + suf, "rb").read() == open(run["lca"] + suf, "rb").read(), suf


def _taxonomy(db_dir):
    nodes, names = {}, {}
    for ln in open(os.path.join(db_dir, "taxonomy", "nodes.dmp")):
        f = [x.strip() for x in ln.split("|")]
        nodes[f[0]] = (f[1], f[2])
    for ln in open(os.path.join(db_dir, "taxonomy", "names.dmp")):
        f = [x.strip() for x in ln.split("|")]
        if f[3] == "scientific name":
            names[f[0]] = f[1]
    return nodes, names


def _recompute(prefix, db_dir, tau):
    """(read IDs, tree ids, parent, depth, lca, mass, near, entries per read) from PREFIX.EM as printed"""
    nodes, _ = _taxonomy(db_dir)
    ids, taxa, post, off = [], [], [], [0]
    for ln in open(prefix + ".EM"):
        f = ln.rstrip("\n").split(" ")
        if not ids or ids[-1] != f[0]:
            if ids:
                off.append(len(post))
            ids.append(f[0])
        taxa.append(re.search(r"kraken:taxid\|(x?\d+)", f[5]).group(1))
        post.append(float(f[13]))
    off.append(len(post))
    depth = {"1": 0}

    def dep(t):
        if t not in depth:
            depth[t] = dep(nodes[t][0]) + 1
        return depth[t]
    for t in set(taxa):
        dep(t)
    tree = sorted(depth, key=lambda t: (depth[t], t))
    index = {t: i for i, t in enumerate(tree)}
    parent = np.array([0] + [index[nodes[t][0]] for t in tree[1:]], dtype=np.int32)
    lca, mass, _, near = lca_ref.assign(parent, off, np.array([index[t] for t in taxa]), np.array(post), tau, margin=1e-4)
    return ids, tree, parent, np.array([depth[t] for t in tree]), lca, mass, near, np.diff(off)


def _kreport(tree, parent, depth, assigned, db_dir, n_total, n_unclassified):
    nodes, names = _taxonomy(db_dir)
    direct = np.bincount(assigned, minlength=len(tree))
    clade = direct.copy()
    kids = [[] for _ in tree]
    for v in range(len(tree) - 1, 0, -1):
        clade[parent[v]] += clade[v]
        kids[parent[v]].append(v)
    out = []
    if n_unclassified:
        out.append("%6.2f\t%d\t%d\tU\t0\tunclassified" % (100.0 * n_unclassified / n_total, n_unclassified, n_unclassified))

    def walk(v):
        if clade[v] == 0:
            return
        code = "R" if v == 0 else CODES.get(nodes[tree[v]][1], "-")
        out.append("%6.2f\t%d\t%d\t%s\t%s\t%s%s" % (100.0 * clade[v] / n_total, clade[v], direct[v], code, tree[v], "  " * int(depth[v]), names[tree[v]]))
        for w in sorted(kids[v], key=lambda w: (-clade[w], tree[w])):
            walk(w)
    walk(0)
    return out


def _meta(prefix):
    return {a: int(b) for a, b in (ln.split() for ln in open(prefix + ".meta"))}


def test_both_files_recomputed_from_the_printed_posteriors(run):
    prefix, tau = run["lca"], 0.8
    ids, tree, parent, depth, lca, mass, near, n_entries = _recompute(prefix, run["db"].dir, tau)
    nodes, _ = _taxonomy(run["db"].dir)
    got = [ln.split("\t") for ln in open(prefix + ".EM.reads2Taxon.lca").read().splitlines()]
    assert [g[0] for g in got] == ids
    assert ids == [ln.split("\t")[0] for ln in open(prefix + ".EM.reads2Taxon").read().splitlines()][:len(ids)]   # the order of reads2Taxon
    print(f"tau {tau}: {int(near.sum())} of {len(ids)} reads within 1e-4 of the threshold")
    assert near.mean() <= 0.02
    index = {t: i for i, t in enumerate(tree)}
    for r, g in enumerate(got):
        assert len(g) == 4 and g[2] == nodes[g[1]][1] and re.fullmatch(r"[01]\.\d{6}", g[3]), g
        if not near[r]:
            assert g[1] == tree[lca[r]], (r, g, tree[lca[r]])
            assert abs(float(g[3]) - mass[r]) <= (n_entries[r] + 1) * 0.5e-6 + 1e-12, (r, g, mass[r])   # half a unit of the printed precision per entry, and of the mass
    assigned = np.where(near, [index[g[1]] for g in got], lca)
    m = _meta(prefix)
    want = _kreport(tree, parent, depth, assigned, run["db"].dir, m["TotalReads"], m["ReadsNotMapped"] + m["ReadsTooShort"])
    assert open(prefix + ".EM.kreport").read().splitlines() == want
    ranks = {g[2] for g in got}
    assert "species" in ranks and "no rank" in ranks                # split reads went up to the species, clear ones stayed on the strain


def test_threshold_one_runs(run):
    prefix = _classify(run, "lca1", ["--lca", "1"])
    _same_old_outputs(run["plain"], prefix)
    got = [ln.split("\t") for ln in open(prefix + ".EM.reads2Taxon.lca").read().splitlines()]
    assert len(got) == len(open(run["lca"] + ".EM.reads2Taxon.lca").read().splitlines())
    assert all(g[3] == "1.000000" for g in got)                     # only a node that holds all of a read's mass qualifies
    rows = [ln.split("\t") for ln in open(prefix + ".EM.kreport").read().splitlines()]
    m = _meta(prefix)
    assert sum(int(r[1]) for r in rows if r[3] in ("U", "R")) == m["TotalReads"]


def test_kreport_invariants(run):
    rows = [ln.split("\t") for ln in open(run["lca"] + ".EM.kreport").read().splitlines()]
    m = _meta(run["lca"])
    assert all(len(r) == 6 and int(r[1]) > 0 for r in rows)
    u = [r for r in rows if r[3] == "U"]
    root = [r for r in rows if r[4] == "1"]
    assert len(root) == 1 and root[0][3] == "R" and len(u) <= 1 and (not u or rows[0] is u[0])
    assert int(root[0][1]) + sum(int(r[1]) for r in u) == m["TotalReads"]
    tree_rows = [r for r in rows if r[3] != "U"]
    ind = [(len(r[5]) - len(r[5].lstrip(" "))) // 2 for r in tree_rows]
    for i, r in enumerate(tree_rows):                              # clade = direct + the clades of the children (the rows one level deeper before the next row of this level or above)
        kids = 0
        for j in range(i + 1, len(tree_rows)):
            if ind[j] <= ind[i]:
                break
            if ind[j] == ind[i] + 1:
                kids += int(tree_rows[j][1])
        assert int(r[1]) == int(r[2]) + kids, r
        assert r[0] == "%6.2f" % (100.0 * int(r[1]) / m["TotalReads"])


@pytest.mark.parametrize("args", [["classify", "--lca", "0.5"], ["classify", "--lca", "1.01"], ["classify", "--lca", "x"], ["classify", "--lca", "-0.8"],
                                  ["classify", "--lca", "8e-1"], ["classify", "--lca", "0.8x"], ["classify", "--lca", "."], ["classify", "--lca"],
                                  ["index", "--lca", "0.8"], ["mapAgainstIndex", "--lca", "0.8"], ["mapDirectly", "--lca", "0.8"]])
def test_refused_forms_of_the_flag(run, args):
    dst = str(run["dir"] / "bad")
    _copy_mappings(run["m"], dst)
    rest = {"classify": ["--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"],
            "index": ["-r", run["db"].fasta, "-i", str(run["dir"] / "idx")],
            "mapAgainstIndex": ["-i", str(run["dir"] / "idx"), "-q", run["q"], "-o", str(run["dir"] / "mai")],
            "mapDirectly": ["--all", "-r", run["db"].fasta, "-q", run["q"], "-o", str(run["dir"] / "md")]}[args[0]]
    p = _run([args[0]] + rest + args[1:])
    assert p.returncode == 1
    assert b"--lca" in p.stderr, p.stderr[-500:]
    for suf in NEW:
        assert not os.path.exists(dst + suf)
