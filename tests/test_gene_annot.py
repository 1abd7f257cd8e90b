"""The parsers of DB_annotations.txt / DB_proteins.faa.annotated and the writers of classify --genes' files (metamaps_amd/csrc/host/gene_annot.hpp),
built without a device as a stand-alone program (tests/test_gene_annot.cpp; plain, and under the address and undefined-behaviour sanitizers) on the
annotated database of tests/gene_db.py, against the text-level restatement of tests/gene_ref.py, byte for byte.  CPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import gene_db
import gene_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SUFFIXES = [".geneLevelAnalysis"] + [".proteins." + t for _, t in gene_ref.TYPES]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("annot") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_gene_annot.cpp")], check=True, timeout=300)
    return p


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    return gene_db.make(str(tmp_path_factory.mktemp("genedb") / "db"), n_genomes=40, genome_len=30_000, seed=7)


def best_mappings(db, n=3000, seed=5):
    """best mappings as a classify run would leave them: random places on the contigs (the one without annotations included), identities with ties"""
    rng = np.random.default_rng(seed)
    sizes = np.array([s.size for s in db.contig_seqs])
    usable = np.flatnonzero(sizes > 3000)[:50]                      # (not every contig is relevant)
    out = []
    for _ in range(n):
        c = int(rng.choice(usable))
        s = int(rng.integers(0, sizes[c] - 2500))
        out.append((db.contig_ids[c], s, s + int(rng.integers(0, 2500)), float(rng.integers(7500, 10001)) / 100 / 100))
    return out


def run(exe, db_dir, prefix, best):
    text = "".join(f"{c}\t{s}\t{e}\t{bits(i)}\n" for c, s, e, i in best)
    p = subprocess.run([exe, db_dir, prefix], input=text.encode(), capture_output=True, timeout=300)
    assert p.returncode in (0, 1), p.stderr.decode()[-2000:]
    return p.returncode, p.stdout.decode().strip()


def variant(db, tmp_path, annotations=None, proteins=None):
    """a copy of the DB's two tables, edited"""
    d = str(tmp_path / "db")
    os.makedirs(d)
    for name, edit in (("DB_annotations.txt", annotations), ("DB_proteins.faa.annotated", proteins)):
        lines = open(os.path.join(db.dir, name)).read().split("\n")
        if edit == "absent":
            continue
        open(os.path.join(d, name), "w").write("\n".join(edit(lines) if edit else lines))
    return d


def check_against_restatement(exe, db_dir, tmp_path, best):
    prefix = str(tmp_path / "out")
    rc, out = run(exe, db_dir, prefix, best)
    assert rc == 0, out
    files, stats = gene_ref.recompute_from_best(best, db_dir)
    for suf in SUFFIXES:
        assert os.path.exists(prefix + suf) == (suf in files), suf
        if suf in files:
            assert open(prefix + suf).read() == files[suf], suf
    word = out.split()
    got = {word[i]: int(word[i + 1]) for i in range(0, len(word), 2)}
    assert got.pop("files") == len(files) - 1
    assert got == stats
    return files, stats


def test_tables_match_the_restatement(exe, db, tmp_path):
    best = best_mappings(db)
    files, stats = check_against_restatement(exe, db.dir, tmp_path, best)
    rows = [ln.split("\t") for ln in files[".geneLevelAnalysis"].splitlines()[1:]]
    names = {r[0] for r in rows}
    assert {"operonA", "rrsA", "dnaA"} <= names and any(r[1] == "" for r in rows) and any(r[2] == "" for r in rows)   # the special genes are met
    assert len(files) == 6 and stats["absent"] == 1 and 0 < stats["annotated_proteins"] < stats["proteins"] and stats["annotated"] == stats["relevant"] - 1
    assert 0 < stats["on"] < stats["reads"]
    assert all(ln.split("\t")[3] == gene_ref.COG[ln.split("\t")[0]] for ln in files[".proteins.COG"].splitlines()[1:])
    both = [b for b in best if b[0].startswith(tuple(r for r in [db.bare_contig]))]
    assert both                                                     # reads on the contig without annotations


def test_columns_in_another_order_and_extra_columns(exe, db, tmp_path):
    def shuffle_columns(perm, extra):
        def edit(lines):
            out = []
            for k, ln in enumerate(lines):
                if not ln:
                    out.append(ln)
                    continue
                f = ln.split("\t")
                f = [f[0]] + [f[i] for i in perm] + ([extra] if k else ["Extra"])
                out.append("\t".join(f))
            return out
        return edit
    d = variant(db, tmp_path, annotations=shuffle_columns([8, 3, 6, 1, 7, 2, 5, 4], "x"), proteins=shuffle_columns([9, 8, 3, 1, 7, 2, 5, 4, 6], ""))
    best = best_mappings(db, n=800, seed=6)
    files, _ = check_against_restatement(exe, d, tmp_path, best)
    (tmp_path / "plain").mkdir()
    same, _ = check_against_restatement(exe, db.dir, tmp_path / "plain", best)
    assert files == same                                            # the order of the columns changes nothing


def test_short_line_in_the_protein_file(exe, db, tmp_path):
    d = variant(db, tmp_path, proteins=lambda lines: lines[:5] + ["\t".join(lines[5].split("\t")[:-1])] + lines[6:])
    rc, out = run(exe, d, str(tmp_path / "o"), best_mappings(db, n=50))
    assert rc == 1 and "DB_proteins.faa.annotated line 6" in out and "fields" in out, out


def test_duplicate_relevant_protein(exe, db, tmp_path):
    best = best_mappings(db, n=2000)
    files, _ = gene_ref.recompute_from_best(best, db.dir)
    met = [r.split("\t")[2] for r in files[".geneLevelAnalysis"].splitlines()[1:] if r.split("\t")[2]]
    lines = open(os.path.join(db.dir, "DB_proteins.faa.annotated")).read().split("\n")
    dup = next(ln for ln in lines[1:] if ln.split("\t")[0] in met)
    d = variant(db, tmp_path, proteins=lambda ls: ls[:-1] + [dup, ""])
    rc, out = run(exe, d, str(tmp_path / "o"), best)
    assert rc == 1 and dup.split("\t")[0] in out and "more than once" in out, out
    (tmp_path / "b").mkdir()                                        # the protein that is in no genome annotation is not relevant: twice is fine
    d2 = variant(db, tmp_path / "b", proteins=lambda ls: ls[:-1] + [next(ln for ln in ls if ln.startswith("WP_999999.1")), ""])
    rc, out = run(exe, d2, str(tmp_path / "o2"), best)
    assert rc == 0 and " absent 2 " in out, out


def test_unknown_cog_letter(exe, db, tmp_path):
    best = best_mappings(db, n=2000)

    def edit(lines):
        out = [lines[0]]
        for ln in lines[1:]:
            f = ln.split("\t")
            if len(f) > 8 and f[8]:
                f[8] = "X, " + f[8]
            out.append("\t".join(f))
        return out
    rc, out = run(exe, variant(db, tmp_path, proteins=edit), str(tmp_path / "o"), best)
    assert rc == 1 and "Unknown COG category X" in out, out


@pytest.mark.parametrize("which", ["DB_annotations.txt", "DB_proteins.faa.annotated"])
def test_missing_file(exe, db, tmp_path, which):
    d = variant(db, tmp_path, **{"annotations" if which == "DB_annotations.txt" else "proteins": "absent"})
    rc, out = run(exe, d, str(tmp_path / "o"), best_mappings(db, n=20))
    assert rc == 1 and which in out and "not found" in out, out
