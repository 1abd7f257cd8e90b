"""`mapDirectly --mods LIST --mod-motifs ...`: PREFIX.motifs.bedmethyl and PREFIX.motifs.tsv beside outputs that stay byte for byte.  The world is that of
tests/test_gpu_cli_mods.py with two contigs: reads written as unaligned BAM with the seeded MM/ML tags of tests/mods_cases.py.  Both files equal what
tests/motif_ref.py computes from the table that the same run's PREFIX.bedmethyl spells out; the same bytes come out with one mm_mod_motifs call per contig
(MM_MOTIF_GROUP_BASES=1), in small batches and with the accumulator merged at every pair; combined strands with their own thresholds (at --mod-min-ml 0, where
PREFIX.bedmethyl shows every entry of the table); a FASTQ query gives the
empty file and the header; the refusals name the flag and the item."""
import numpy as np
import pytest

import bam_writer as bw
import mods_cases
import mods_ref
import motif_ref
from test_gpu_cli_edit_distance import _run, _take
from test_gpu_cli_mods import CODE_NAME, LIST, tags_of

pytestmark = pytest.mark.gpu
MOTIFS = [("GATC", 1), ("CCWGG", 1), ("CG", 0)]
ITEMS = ",".join("%s:%d" % m for m in MOTIFS)
COMBINED = [("CG", 0), ("GATC", 1)]
CODE_BASE = "CCA"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("motifcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11, contigs_per_genome=1, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=100, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    reads = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 4)}
    even = [c for g in range(0, len(db.genome_contigs), 2) for c in db.genome_contigs[g]]
    cname, contigs = [db.contig_ids[c].split()[0] for c in even], [db.contig_seqs[c].tobytes().upper() for c in even]
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for c in even:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    rng = np.random.default_rng(406)
    records = []
    for k, (name, read) in enumerate(reads.items()):
        tags = b"" if k % 7 == 3 else tags_of(mods_cases.dense_groups(rng, read), k % 3 == 0)
        records.append(bw.record_bytes(name, read.decode().upper(), 0x10 if k % 4 == 1 else 0, tags=tags))
    bam = str(d / "r.bam")
    bw.write_bgzf(bam, bw.header_bytes() + b"".join(records))
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", fasta, "-q", bam, "-o", prefix, "--mods", LIST]
    # (a unit's N_fail holds its partner's failed calls even where the partner has nothing else and PREFIX.bedmethyl no row of it: at --mod-min-ml 0 no call fails)
    comb = ["--mod-motifs", ",".join("%s:%d" % m for m in COMBINED), "--mod-motif-combine-strands", "--mod-motif-min-frac", "0.3", "--mod-min-coverage", "2", "--mod-min-ml", "0"]
    runs = {}
    for tag, extra, env in (("mods", ["--paf"], None), ("mods_ml0", ["--mod-min-ml", "0"], None), ("motifs", ["--paf", "--mod-motifs", ITEMS], None), ("groups", ["--mod-motifs", ITEMS], {"MM_MOTIF_GROUP_BASES": "1"}),
                            ("batches", ["--mod-motifs", ITEMS], {"MM_CLI_BATCH_READS": "5"}), ("merges", ["--mod-motifs", ITEMS], {"MM_MODS_MERGE_PAIRS": "1"}),
                            ("combined", comb, None), ("combined_groups", comb, {"MM_MOTIF_GROUP_BASES": "1"})):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(cname=cname, contigs=contigs, runs=runs, fasta=fasta, fastq=rd["path"], bam=bam, dir=d)


def table_of(bedmethyl, cname):
    """the merged table that a PREFIX.bedmethyl written with --mod-min-coverage 1 spells out (sites of failed calls alone, which no row shows, are covered nowhere)"""
    sites = {}
    for ln in bedmethyl.decode().splitlines():
        f = ln.split("\t")
        sites.setdefault((cname.index(f[0]), int(f[1]), 1 if f[5] == "+" else -1), {})[CODE_NAME.index(f[3])] = [int(f[x]) for x in (11, 12, 13, 15)]
    t = {}
    for (c, pos, strand), rows in sites.items():
        k, (n_mod, n_canon, n_other, n_fail) = next(iter(rows.items()))
        cnt = {0: n_canon, 1: n_fail, 2: n_other - sum(r[0] for o, r in rows.items() if o != k)}
        cnt.update({3 + o: r[0] for o, r in rows.items()})
        assert cnt[2] >= 0 and all(r[1] == n_canon and r[3] == n_fail for r in rows.values())
        t.update({mods_ref.key(c, pos, strand, cls): n for cls, n in cnt.items() if n})
    return t


def expected(world, motifs, min_coverage=1, min_frac=0.5, combine=False, base="mods"):
    t = table_of(world["runs"][base][".bedmethyl"], world["cname"])
    rows, summary = motif_ref.profile(world["contigs"], t, CODE_BASE, motifs, min_coverage, min_frac, combine)
    return motif_ref.bedmethyl_text(rows, world["cname"], CODE_NAME, motifs), motif_ref.tsv_text(summary, world["cname"], CODE_NAME, motifs), rows, summary


def test_both_files_equal_the_restatement(world):
    run = world["runs"]["motifs"]
    bed, tsv, rows, summary = expected(world, MOTIFS)
    assert run[".motifs.bedmethyl"] == bed and run[".motifs.tsv"] == tsv
    assert len(rows) > 1000 and {r[3] for r in rows} == {0, 1, 2} and {r[2] for r in rows} == {1, -1} and {r[4] for r in rows} == {0, 1, 2}
    assert {s[0] for s in summary} == {0, 1} and any(s[5] for s in summary) and all(s[3] >= s[4] for s in summary) and any(s[3] > s[4] > 0 for s in summary)   # both contigs; occurrences without coverage too
    cols = run[".motifs.bedmethyl"].decode().splitlines()[0].split("\t")
    assert len(cols) == 18 and cols[3].split(",")[1:] in (["GATC", "1"], ["CCWGG", "1"], ["CG", "0"]) and cols[8] == "255,0,0"
    assert run[".motifs.tsv"].decode().splitlines()[-1].startswith("*\tCG\t0\t")
    # every other file, PREFIX.bedmethyl included, is the file of the run without the flag
    plain = world["runs"]["mods"]
    assert set(run) == set(plain) | {".motifs.bedmethyl", ".motifs.tsv"}
    for suf in plain:
        assert run[suf] == plain[suf], suf


def test_groups_batches_and_merges_do_not_change_a_byte(world):
    want = world["runs"]["motifs"]
    for tag in ("groups", "batches", "merges"):
        for suf in (".motifs.bedmethyl", ".motifs.tsv", ".bedmethyl"):
            assert world["runs"][tag][suf] == want[suf], (tag, suf)


def test_combined_strands_and_thresholds(world):
    run = world["runs"]["combined"]
    bed, tsv, rows, summary = expected(world, COMBINED, 2, 0.3, True, "mods_ml0")
    assert run[".motifs.tsv"] == tsv
    assert run[".motifs.bedmethyl"].splitlines() == bed.splitlines() and run[".motifs.bedmethyl"] == bed and len(rows) > 300
    assert {ln.split("\t")[5] for ln in bed.decode().splitlines()} == {"."}
    for suf in (".motifs.bedmethyl", ".motifs.tsv"):
        assert world["runs"]["combined_groups"][suf] == run[suf], suf


def test_a_fastq_query_gives_the_empty_file_and_the_header(world):
    prefix = str(world["dir"] / "fq")
    p = _run(["mapDirectly", "-r", world["fasta"], "-q", world["fastq"], "-o", prefix, "--mods", LIST, "--mod-motifs", ITEMS])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = _take(prefix)
    assert got[".motifs.bedmethyl"] == b"" and got[".motifs.tsv"] == motif_ref.TSV_HEADER.encode() and got[".bedmethyl"] == b"" and len(got[""]) > 1000


def test_refusals_name_the_flag_and_the_item(world, tmp_path):
    base = ["-r", world["fasta"], "-q", world["bam"], "-o", str(tmp_path / "o")]
    mods = ["--mods", LIST]
    for mode, extra, what in (("mapDirectly", mods + ["--mod-motifs", ITEMS, "--hpc"], "--mod-motifs cannot be combined with --hpc"),
                              ("mapDirectly", mods + ["--mod-motifs", ITEMS, "--shard-index"], "--mod-motifs cannot be combined with --shard-index or --stream-chunks"),
                              ("mapAgainstIndex", mods + ["--mod-motifs", ITEMS], "--mod-motifs belongs to mapDirectly"),
                              ("mapDirectly", ["--mod-motifs", ITEMS], "--mod-motifs needs --mods"),
                              ("mapDirectly", ["--mod-motif-min-frac", "0.5"], "--mod-motif-min-frac needs --mods"),
                              ("mapDirectly", ["--mod-motif-combine-strands"], "--mod-motif-combine-strands needs --mods"),
                              ("mapDirectly", mods + ["--mod-motif-min-frac", "0.5"], "--mod-motif-min-frac needs --mod-motifs"),
                              ("mapDirectly", mods + ["--mod-motif-combine-strands"], "--mod-motif-combine-strands needs --mod-motifs"),
                              ("mapDirectly", mods + ["--mod-motifs", "GATC:1,gatc:1"], "--mod-motifs takes 1 to 8 comma-separated items MOTIF:OFFSET"),
                              ("mapDirectly", mods + ["--mod-motifs", "GATC:1,gatc:1"], "not 'gatc:1'"),
                              ("mapDirectly", mods + ["--mod-motifs", "GATC"], "not 'GATC'"),
                              ("mapDirectly", mods + ["--mod-motifs", "GAXC:1"], "not 'GAXC:1'"),
                              ("mapDirectly", mods + ["--mod-motifs", "C" * 33 + ":0"], "--mod-motifs takes 1 to 8"),
                              ("mapDirectly", mods + ["--mod-motifs", ",".join("C" * n + ":0" for n in range(1, 10))], "not 'CCCCCCCCC:0'"),
                              ("mapDirectly", mods + ["--mod-motifs", "CG:0,,GATC:1"], "not ''"),
                              ("mapDirectly", mods + ["--mod-motifs", "GATC:4"], "--mod-motifs: the item GATC:4: the offset 4 is not inside the motif's 4 letters"),
                              ("mapDirectly", mods + ["--mod-motifs", "GANTC:2"], "--mod-motifs: the item GANTC:2: the modified base N is not one of A C G T"),
                              ("mapDirectly", mods + ["--mod-motifs", "GATC:2"], "--mod-motifs: the item GATC:2: no code of --mods has the base T"),
                              ("mapDirectly", mods + ["--mod-motifs", "CG:0,GATC:1,CG:0"], "--mod-motifs: the item CG:0 is given twice"),
                              ("mapDirectly", mods + ["--mod-motifs", ITEMS, "--mod-motif-min-frac", "1.5"], "--mod-motifs: --mod-motif-min-frac takes a decimal from 0 to 1, not '1.5'"),
                              ("mapDirectly", mods + ["--mod-motifs", ITEMS, "--mod-motif-min-frac", "x"], "--mod-motifs: --mod-motif-min-frac takes a decimal from 0 to 1, not 'x'"),
                              ("mapDirectly", mods + ["--mod-motifs", "CG:0,GGTGA:4,CCAGG:1", "--mod-motif-combine-strands"],
                               "--mod-motif-combine-strands: the motif GGTGA is not its own reverse complement")):
        p = _run([mode] + base + extra)
        assert p.returncode == 1 and what in p.stderr.decode(), (extra, p.stderr.decode()[-500:])
        assert _take(str(tmp_path / "o")) == {}                     # before any work
