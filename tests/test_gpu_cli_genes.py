"""`classify --genes` and `mapDirectly --then-classify --genes`: PREFIX.EM.geneLevelAnalysis and PREFIX.EM.proteins.TYPE beside unchanged outputs, both
recomputed byte for byte in Python from PREFIX.EM and the DB's two annotation tables (tests/gene_ref.py) on the annotated database of tests/gene_db.py;
the same files from two logical devices, through --then-classify and behind --hpc mappings; a missing annotation table; the refusals of the flag."""
import os
import shutil
import subprocess

import pytest

import gene_db
import gene_ref
from test_gpu_cli import CLI
from test_gpu_cli_bootstrap import OUTS, _copy_mappings

pytestmark = pytest.mark.gpu
NEW = [".EM.geneLevelAnalysis"] + [".EM.proteins." + t for _, t in gene_ref.TYPES]


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=900)


def _classify(run, tag, extra):
    dst = str(run["dir"] / tag)
    _copy_mappings(run["m"], dst)
    p = _run(["classify", "--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"] + extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dst, p.stdout.decode()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("genes")
    db = gene_db.make(str(d / "db"), n_genomes=40, genome_len=30_000, seed=7)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=2000, read_len=3000, seed=3, abundance_sigma=0.5)   # (even enough that every large contig gets reads)
    out = {"dir": d, "db": db, "q": rd["path"], "m": str(d / "map0")}
    p = _run(["mapDirectly", "--all", "-r", db.fasta, "-q", rd["path"], "-o", out["m"]])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out["plain"], _ = _classify(out, "plain", [])
    out["genes"], out["stdout"] = _classify(out, "genes", ["--genes"])
    return out


def _same_old_outputs(a, b):
    for suf in OUTS:
        assert os.path.exists(a + suf) == os.path.exists(b + suf), suf
        if os.path.exists(a + suf):
            assert open(a + suf, "rb").read() == open(b + suf, "rb").read(), suf
    assert os.path.exists(a + ".EM") and os.path.exists(a + ".EM.WIMP")


def _matches_restatement(prefix, db_dir):
    files, stats = gene_ref.recompute(prefix, db_dir)
    for suf in NEW:
        assert os.path.exists(prefix + suf) == (suf[3:] in files), suf
        if suf[3:] in files:
            assert open(prefix + suf).read() == files[suf[3:]], suf
    return files, stats


def test_old_outputs_unchanged_and_no_new_file_without_the_flag(run):
    _same_old_outputs(run["plain"], run["genes"])
    for suf in NEW:
        assert not os.path.exists(run["plain"] + suf), suf


def test_files_equal_the_text_level_restatement(run):
    files, stats = _matches_restatement(run["genes"], run["db"].dir)
    assert len(files) == 6                                          # the gene table and all five annotation types
    rows = [ln.split("\t") for ln in files[".geneLevelAnalysis"].splitlines()[1:]]
    assert len(rows) > 100 and any(int(r[4]) >= 10 for r in rows) and any(r[1] == "" for r in rows)
    assert 0 < stats["on"] < stats["reads"] and stats["annotated"] < stats["relevant"]      # reads on the contig without annotations
    text = run["stdout"]
    assert f"found {stats['relevant']} relevant contig IDs, of which we have annotations for {stats['annotated']}." in text
    assert f"Of {stats['reads']} mapped reads, {stats['on']} go to contigs with annotations and {stats['reads'] - stats['on']} to contigs without." in text
    assert f"Found {stats['genes']} genes and {stats['proteins']} proteins, of which {stats['annotated_proteins']} carry any type of additional annotation." in text
    assert f"% of a total of {stats['protein_lines']} in the protein annotations are not in the genome annotations." in text and stats["absent"] == 1


def test_then_classify_writes_the_same_files(run):
    o = str(run["dir"] / "direct")
    p = _run(["mapDirectly", "--all", "-r", run["db"].fasta, "-q", run["q"], "-o", o, "--then-classify", run["db"].dir, "--minreads", "3", "--genes"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    _same_old_outputs(run["plain"], o)
    for suf in NEW:
        assert open(o + suf, "rb").read() == open(run["genes"] + suf, "rb").read(), suf


def test_two_logical_devices_write_the_same_files(run):
    two, _ = _classify(run, "two", ["--genes", "--devices", "0,0", "--em-host-reduce"])   # the analysis runs on the first device, for all reads
    _same_old_outputs(run["plain"], two)
    for suf in NEW:
        assert open(two + suf, "rb").read() == open(run["genes"] + suf, "rb").read(), suf


def test_behind_hpc_mappings(run):
    o = str(run["dir"] / "hpc")
    p = _run(["mapDirectly", "--all", "--hpc", "-r", run["db"].fasta, "-q", run["q"], "-o", o, "--then-classify", run["db"].dir, "--minreads", "3", "--genes"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    files, stats = _matches_restatement(o, run["db"].dir)           # the reported coordinates are raw: the restatement of its own .EM
    assert stats["genes"] > 100


@pytest.mark.parametrize("which", ["DB_annotations.txt", "DB_proteins.faa.annotated"])
def test_missing_annotation_file(run, tmp_path, which):
    db2 = str(tmp_path / "db")
    shutil.copytree(run["db"].dir, db2)
    os.remove(os.path.join(db2, which))
    dst = str(tmp_path / "m")
    _copy_mappings(run["m"], dst)
    p = _run(["classify", "--DB", db2, "--mappings", dst, "--minreads", "3", "--genes"])
    assert p.returncode == 1 and which in p.stderr.decode(), p.stderr[-500:]
    assert not os.path.exists(dst + ".EM")                          # before any work
    p = _run(["mapDirectly", "--all", "-r", run["db"].fasta, "-q", run["q"], "-o", str(tmp_path / "d"), "--then-classify", db2, "--genes"])
    assert p.returncode == 1 and which in p.stderr.decode() and not os.path.exists(str(tmp_path / "d"))


@pytest.mark.parametrize("mode", ["index", "mapAgainstIndex", "mapDirectly"])
def test_refused_forms_of_the_flag(run, mode):
    rest = {"index": ["-r", run["db"].fasta, "-i", str(run["dir"] / "idx")],
            "mapAgainstIndex": ["-i", str(run["dir"] / "idx"), "-q", run["q"], "-o", str(run["dir"] / "mai")],
            "mapDirectly": ["--all", "-r", run["db"].fasta, "-q", run["q"], "-o", str(run["dir"] / "md")]}[mode]
    p = _run([mode] + rest + ["--genes"])
    assert p.returncode == 1
    assert b"--genes needs classify or mapDirectly --then-classify" in p.stderr, p.stderr[-500:]
    assert not os.path.exists(str(run["dir"] / "md")) and not os.path.exists(str(run["dir"] / "idx"))
