"""`mapDirectly --paf`: PREFIX.paf beside the outputs of a run with --edit-distance, which stay byte for byte — one PAF line per ALIGNED line of PREFIX in
the same order, twelve columns and the tags NM and cg, the CIGAR equal to the naive suffix table's walk (tests/edit_cigar_ref.py) on that line's read and
contig window, the coordinates and NM those of the .editDistances line; the same with --all --then-classify (the .EM* files unchanged), and from two
logical devices in small batches with --compress-output; the refused combinations name --paf."""
import glob
import re

import pytest

import edit_cigar_ref
import edit_ref
from test_gpu_cli import CLASSIFY_SUFFIXES
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("pafcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=24, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    reads = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 4)}
    contigs = {cid.split()[0]: seq.tobytes() for cid, seq in zip(db.contig_ids, db.contig_seqs)}
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", db.fasta, "-q", rd["path"], "-o", prefix]
    runs = {}
    for tag, extra, env in (("best_ed", ["--edit-distance"], None), ("best_paf", ["--paf"], None),
                            ("all_ed", ["--all", "--then-classify", db.dir, "--minreads", "3", "--edit-distance"], None),
                            ("all_paf", ["--all", "--then-classify", db.dir, "--minreads", "3", "--paf"], None),
                            ("all_paf_two", ["--all", "--paf", "--compress-output", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"})):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, contigs=contigs, runs=runs, dir=d, q=rd["path"], memo={})


def _check_paf(world, run):
    maps, eds, paf = run[""].decode().splitlines(), run[".editDistances"].decode().splitlines(), run[".paf"].decode().splitlines()
    assert len(maps) == len(eds)
    it, aligned, edits = iter(paf), 0, 0
    for m, e in zip(maps, eds):
        f, g = m.split(" "), e.split(" ")
        if g[3] == "NA":                                           # not aligned: no PAF line (the next one belongs to the next aligned mapping)
            continue
        c = next(it).split("\t")
        assert len(c) == 14 and c[12].startswith("NM:i:") and c[13].startswith("cg:Z:"), c[:13]
        read, contig, strand = world["reads"][f[0]], world["contigs"][f[5]], 1 if f[4] == "+" else -1
        assert c[:7] == [f[0], str(len(read)), "0", str(len(read)), f[4], f[5], str(len(contig))], (m, c[:12])
        assert [c[7], str(int(c[8]) - 1), c[12][5:]] == [g[4], g[5], g[3]], (e, c[:13])
        key = (f[0], f[5], f[4], f[7])
        if key not in world["memo"]:
            ws, we = edit_ref.window(int(f[7]), len(read), len(contig))
            world["memo"][key] = edit_cigar_ref.align(read, strand, contig[ws:we], edit_ref.cap(len(read)))
        want = world["memo"][key]
        assert want is not None and c[13][5:] == edit_cigar_ref.cigar(want[3]), (m, c[13][:200])
        runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", c[13][5:])]
        assert "".join(f"{n}{op}" for n, op in runs) == c[13][5:]
        assert int(c[9]) == sum(n for n, op in runs if op == "=") and int(c[10]) == sum(n for n, op in runs) and c[11] == "255"
        aligned += 1
        edits += want[0] > 0
    assert next(it, None) is None                                  # no line beyond the aligned mappings
    assert aligned >= 15 and edits >= 10
    return aligned, len(maps)


def test_best_mappings(world):
    a, b = world["runs"]["best_ed"], world["runs"]["best_paf"]
    assert ".paf" not in a and set(b) == set(a) | {".paf"}
    for suf in SAME + (".editDistances",):
        assert a[suf] == b[suf], suf
    _check_paf(world, b)


def test_all_mappings_and_then_classify(world):
    a, b = world["runs"]["all_ed"], world["runs"]["all_paf"]
    assert set(b) == set(a) | {".paf"}
    for suf in SAME + CLASSIFY_SUFFIXES + (".editDistances",):
        assert a[suf] == b[suf], suf
    assert len(a[".EM.WIMP"]) > 100
    aligned, lines = _check_paf(world, b)
    assert aligned < lines                                         # some mapping of --all is not aligned (NA NA NA): it has no PAF line


def test_two_devices_small_batches_compressed(world):
    """every device traces the batches it mapped: the lines come out in the order of PREFIX whichever device made them, and PREFIX.paf stays plain"""
    a, b = world["runs"]["all_paf"], world["runs"]["all_paf_two"]
    assert ".gz" in b and "" not in b
    assert b[".paf"] == a[".paf"] and b[".editDistances"] == a[".editDistances"] and b[".meta"] == a[".meta"]


def test_refused_combinations(world, tmp_path):
    db, q, x = world["db"], world["q"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["all_paf"][""])
    for args in (["mapDirectly", "--paf", "--hpc", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--paf", "--shard-index", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--paf", "--stream-chunks", "--maxmemory-bytes", "100000", "-r", db.fasta, "-q", q, "-o", x],
                 ["index", "--paf", "-r", db.fasta, "-i", x],
                 ["mapAgainstIndex", "--paf", "-i", x, "-q", q, "-o", x],
                 ["classify", "--paf", "--DB", db.dir, "--mappings", maps]):
        p = _run(args)
        assert p.returncode == 1 and "--paf" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
