"""`mapDirectly --bam`: PREFIX.bam beside the outputs of the same run without the flag, which stay byte for byte.  The file is read whole by the
independent decoder of tests/bam_ref.py: the header and reference list of the DB's contigs, one record per line of PREFIX.paf in order and equal to
it field by field (name, strand bit, refID, pos, CIGAR, NM), the bin, SEQ the read or its reverse complement, QUAL 0xFF, MD rebuilding the contig
under the alignment, mapq recomputed from field 14 of the record's own line of PREFIX, one primary record per read and the one the rule names; with
--all --then-classify, from two logical devices in small batches with --compress-output, back through the product's own BAM reader, and the refused
combinations."""
import glob
import gzip
import os

import pytest

import bam_ref
import edit_ref
from test_gpu_cli import CLASSIFY_SUFFIXES
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("bamcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=24, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    reads = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 4)}
    contigs = [(cid.split()[0], seq.tobytes()) for cid, seq in zip(db.contig_ids, db.contig_seqs)]
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", db.fasta, "-q", rd["path"], "-o", prefix]
    classify = ["--all", "--then-classify", db.dir, "--minreads", "3"]
    runs = {}
    for tag, extra, env in (("paf", ["--paf"], None), ("paf_bam", ["--paf", "--bam"], None), ("bam", ["--bam"], None),
                            ("all_paf", classify + ["--paf"], None), ("all_paf_bam", classify + ["--paf", "--bam"], None),
                            ("all_bam_two", ["--all", "--bam", "--compress-output", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"})):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, contigs=contigs, runs=runs, dir=d, q=rd["path"], base=base, prefix=prefix)


def _check_bam(world, run, paf):
    """the .bam of a run against the lines of PREFIX and of a PREFIX.paf of the same mappings"""
    text, refs, recs = bam_ref.decode(run[".bam"])
    names = [n for n, _ in world["contigs"]]
    assert text == bam_ref.HD_LINE + "".join(f"@SQ\tSN:{n}\tLN:{len(s)}\n" for n, s in world["contigs"]) + bam_ref.PG_LINE
    assert refs == [(n, len(s)) for n, s in world["contigs"]]
    maps, eds, paf = run[""].decode().splitlines(), run[".editDistances"].decode().splitlines(), paf.decode().splitlines()
    assert len(recs) == len(paf) and len(maps) == len(eds)
    it, best, edits = iter(zip(recs, paf)), {}, 0
    for k, (m, e) in enumerate(zip(maps, eds)):
        f, g = m.split(" "), e.split(" ")
        if g[3] == "NA":                                           # not aligned: no record
            continue
        r, c = next(it)
        c = c.split("\t")
        first, last, d = int(g[4]), int(g[5]), int(g[3])
        assert (r["name"].decode(), bool(r["flag"] & 0x10), names[r["refID"]]) == (f[0], f[4] == "-", f[5]) == (c[0], c[4] == "-", c[5]), (m, r)
        assert r["flag"] & ~0x110 == 0 and r["pos"] == int(c[7]) == first and (r["next_refID"], r["next_pos"], r["tlen"]) == (-1, -1, 0)
        assert bam_ref.cigar_string(r["cigar"]) == c[13][5:] and r["cigar_field"] == r["cigar"] and r["tags"]["NM"] == d == int(c[12][5:])
        assert r["tag_order"] == ["NM", "MD"] and r["bin"] == bam_ref.reg2bin(first, last + 1)
        read = world["reads"][f[0]]
        assert r["seq"] == edit_ref.oriented(read, -1 if f[4] == "-" else 1).decode().upper() and r["l_seq"] == len(read) and r["qual"] == b"\xff" * len(read)
        contig = dict(world["contigs"])[f[5]]
        assert bam_ref.ref_from_md(r["seq"], r["cigar"], r["tags"]["MD"]) == contig[first:last + 1].decode().upper(), m
        assert r["mapq"] == bam_ref.mapq_from_text(f[13]), (m, r["mapq"])
        q = float(f[13])
        if f[0] not in best or q > best[f[0]][0]:                    # the largest field 14 among the read's aligned lines, the first of equals
            best[f[0]] = (q, k)
        r["line"] = k
        edits += d > 0
    assert next(it, None) is None
    primary = {}
    for r in recs:
        if not r["flag"] & 0x100:
            assert r["name"].decode() not in primary, "two primary records of one read"
            primary[r["name"].decode()] = r["line"]
    assert primary == {n: k for n, (_, k) in best.items()}
    assert len(recs) >= 15 and edits >= 10
    return len(recs), len(maps), primary


def test_best_mappings(world):
    a, b, c = world["runs"]["paf"], world["runs"]["paf_bam"], world["runs"]["bam"]
    assert ".bam" not in a and set(b) == set(a) | {".bam"} and set(c) == set(a) - {".paf"} | {".bam"}
    for suf in SAME + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
        assert suf == ".paf" or a[suf] == c[suf], suf
    _check_bam(world, b, b[".paf"])
    assert gzip.decompress(c[".bam"]) == gzip.decompress(b[".bam"])


def test_all_mappings_and_then_classify(world):
    a, b = world["runs"]["all_paf"], world["runs"]["all_paf_bam"]
    assert set(b) == set(a) | {".bam"}
    for suf in SAME + CLASSIFY_SUFFIXES + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    n_rec, n_lines, primary = _check_bam(world, b, b[".paf"])
    assert n_rec < n_lines                                          # some mapping of --all is not aligned: it has no record
    assert n_rec > len(primary)                                     # reads with secondary records


def test_two_devices_small_batches_compressed(world):
    """every device encodes the batches it mapped; the members come out in the order of PREFIX; the same stream as from one device"""
    a, b = world["runs"]["all_paf_bam"], world["runs"]["all_bam_two"]
    assert ".gz" in b and "" not in b and ".paf" not in b
    assert gzip.decompress(b[".gz"]) == a[""] and b[".editDistances"] == a[".editDistances"] and b[".meta"] == a[".meta"]
    assert b[".bam"].endswith(bam_ref.EOF_BLOCK) and gzip.decompress(b[".bam"]) == gzip.decompress(a[".bam"])
    assert len(bam_ref.members(b[".bam"])) > len(bam_ref.members(a[".bam"]))   # five batches: a member each at least


def test_round_trip_through_the_bam_reader(world):
    """mapDirectly -q PREFIX.bam: the primary records are the reads again (strand - turned back), and map as they did"""
    run = world["runs"]["bam"]
    path = str(world["dir"] / "again.bam")
    open(path, "wb").write(run[".bam"])
    base = list(world["base"])
    base[base.index("-q") + 1] = path
    p = _run(base)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    again = _take(world["prefix"])
    os.remove(path)
    recs = bam_ref.decode(run[".bam"])[2]
    have = {r["name"].decode() for r in recs if not r["flag"] & 0x100}
    want = [m for m in run[""].decode().splitlines() if m.split(" ")[0] in have]
    assert len(have) >= 15 and again[""].decode().splitlines() == want


def test_refused_combinations(world, tmp_path):
    db, q, x = world["db"], world["q"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["all_paf_bam"][""])
    for args in (["mapDirectly", "--bam", "--hpc", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--bam", "--paf", "--shard-index", "-r", db.fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--bam", "--stream-chunks", "--maxmemory-bytes", "100000", "-r", db.fasta, "-q", q, "-o", x],
                 ["index", "--bam", "-r", db.fasta, "-i", x],
                 ["mapAgainstIndex", "--bam", "-i", x, "-q", q, "-o", x],
                 ["classify", "--bam", "--DB", db.dir, "--mappings", maps]):
        p = _run(args)
        assert p.returncode == 1 and "--bam" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
