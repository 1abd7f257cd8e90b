"""`mapDirectly --edit-distance`: PREFIX.editDistances beside outputs that are byte for byte those of a run without the flag — one line per line of PREFIX in
the same order, `readID contigID strand d first last`, the numbers equal to the naive dynamic programme's (tests/edit_ref.py: record) on the read and contig
of that line; the same with --all, with --then-classify (the .EM* files unchanged), and from two logical devices in small batches with --compress-output;
the refused combinations."""
import glob
import os
import subprocess

import pytest

import edit_ref
from test_gpu_cli import CLI, CLASSIFY_SUFFIXES

pytestmark = pytest.mark.gpu
SAME = ("", ".meta", ".meta.unmappedReadsLengths", ".parameters")


def _run(args, env=None):
    return subprocess.run([CLI] + args, capture_output=True, timeout=600, env=dict(os.environ, **(env or {})))


def _take(prefix):
    """the files of a run by suffix, removed from the disk (the next run writes the same prefix: PREFIX.parameters names it)"""
    out = {}
    for f in glob.glob(prefix + "*"):
        out[f[len(prefix):]] = open(f, "rb").read()
        os.remove(f)
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("editcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=24, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    reads = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 4)}
    contigs = {cid.split()[0]: seq.tobytes() for cid, seq in zip(db.contig_ids, db.contig_seqs)}
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", db.fasta, "-q", rd["path"], "-o", prefix]
    runs = {}
    for tag, extra, env in (("best", [], None), ("best_ed", ["--edit-distance"], None),
                            ("all", ["--all", "--then-classify", db.dir, "--minreads", "3"], None),
                            ("all_ed", ["--all", "--then-classify", db.dir, "--minreads", "3", "--edit-distance"], None),
                            ("all_ed_two", ["--all", "--edit-distance", "--compress-output", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"})):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, contigs=contigs, runs=runs, dir=d, q=rd["path"], memo={})


def _check_lines(world, run):
    maps, eds = run[""].decode().splitlines(), run[".editDistances"].decode().splitlines()
    assert len(maps) == len(eds) and len(maps) >= 15
    aligned = 0
    for m, e in zip(maps, eds):
        f, g = m.split(" "), e.split(" ")
        assert len(g) == 6 and g[:3] == [f[0], f[5], f[4]], (m, e)
        key = (f[0], f[5], f[4], f[7])
        if key not in world["memo"]:
            world["memo"][key] = edit_ref.record(world["reads"][f[0]], 1 if f[4] == "+" else -1, world["contigs"][f[5]], int(f[7]))
        want = world["memo"][key]
        assert g[3:] == (["NA", "NA", "NA"] if want is None else [str(x) for x in want]), (m, e, want)
        aligned += want is not None
    assert aligned >= 15


def test_best_mappings(world):
    a, b = world["runs"]["best"], world["runs"]["best_ed"]
    assert ".editDistances" not in a and set(b) == set(a) | {".editDistances"}
    for suf in SAME:
        assert a[suf] == b[suf], suf
    _check_lines(world, b)


def test_all_mappings_and_then_classify(world):
    a, b = world["runs"]["all"], world["runs"]["all_ed"]
    assert set(b) == set(a) | {".editDistances"}
    for suf in SAME + CLASSIFY_SUFFIXES:
        assert a[suf] == b[suf], suf
    assert len(a[".EM.WIMP"]) > 100
    _check_lines(world, b)


def test_two_devices_small_batches_compressed(world):
    """every device aligns the batches it mapped: the lines come out in the order of PREFIX whichever device made them"""
    a, b = world["runs"]["all_ed"], world["runs"]["all_ed_two"]
    assert ".gz" in b and "" not in b
    assert b[".editDistances"] == a[".editDistances"] and b[".meta"] == a[".meta"]


def test_refused_combinations(world, tmp_path):
    db, q, x = world["db"], world["q"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["all"][""])
    for args in (["mapDirectly", "--edit-distance", "--hpc", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--edit-distance", "--shard-index", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--edit-distance", "--stream-chunks", "--maxmemory-bytes", "100000", "-r", db.fasta, "-q", q, "-o", x],
                 ["index", "--edit-distance", "-r", db.fasta, "-i", x],
                 ["mapAgainstIndex", "--edit-distance", "-i", x, "-q", q, "-o", x],
                 ["classify", "--edit-distance", "--DB", db.dir, "--mappings", maps]):
        p = _run(args)
        assert p.returncode == 1 and "--edit-distance" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
