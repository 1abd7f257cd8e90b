"""`mapDirectly --mods`: PREFIX.bedmethyl beside outputs that stay byte for byte.  The world is that of tests/test_gpu_cli_pileup.py (one genome as the
reference, reads from it and from its 3 % substitution copy) with the reads written as unaligned BAM carrying seeded C+m?, C+h?, A+a. and G+o? groups
(every third read with the two C codes in one group, C+mh?; BAM carries no case, so the reads go in upper case), some records reverse-complemented (0x10), every seventh without tags, one with an MN that
differs from its length.  The file equals what tests/mods_ref.py computes from the same run's PREFIX (field 14 gives a read's primary record),
.editDistances and .paf and the BAM's tags; the same bytes come out under two logical devices in small batches, with the accumulator merged every 50
pairs and with --bam --pileup added; a FASTQ query gives an empty file and an INFO line; a malformed tag ends the run with the read's name; the refused
combinations name --mods."""
import struct

import numpy as np
import pytest

import bam_writer as bw
import mods_cases
import mods_ref
from test_gpu_cli_edit_distance import _run, _take
from test_gpu_cli_pileup import _jobs

pytestmark = pytest.mark.gpu
LIST = "C+m,C+h,A+a"
CODE_NAME, CODE_BASE = ["m", "h", "a"], ["C", "C", "A"]


def tags_of(groups, combined, mn=None):
    """the MM, ML (and MN) fields of mods_cases.dense_groups' four groups; combined: the two C codes as one group C+mh? with interleaved ML bytes"""
    m, h, a, g = groups
    text = lambda head, grp: head + "".join(",%d" % s for s in grp["skips"]) + ";"
    if combined:
        assert m["skips"] == h["skips"]
        mm = text("C+mh?", m) + text("A+a.", a) + text("G+o?", g)
        ml = [x for pair in zip(m["ml"], h["ml"]) for x in pair] + a["ml"] + g["ml"]
    else:
        mm = text("C+m?", m) + text("C+h?", h) + text("A+a.", a) + text("G+o?", g)
        ml = m["ml"] + h["ml"] + a["ml"] + g["ml"]
    t = b"MMZ" + mm.encode() + b"\0" + b"MLBC" + struct.pack("<I", len(ml)) + bytes(ml)
    return t + (b"MNi" + struct.pack("<i", mn) if mn is not None else b"")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("modscli")
    db = synth.make_db(str(d / "db"), n_genomes=2, genome_len=30_000, seed=11, contigs_per_genome=1, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=150, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    reads = {lines[i][1:].split()[0].decode(): lines[i + 1] for i in range(0, len(lines) - 1, 4)}
    even = [c for g in range(0, len(db.genome_contigs), 2) for c in db.genome_contigs[g]]
    cname, contigs = [db.contig_ids[c].split()[0] for c in even], [db.contig_seqs[c].tobytes() for c in even]
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for c in even:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    rng = np.random.default_rng(405)
    planes, records = {}, []
    for k, (name, read) in enumerate(reads.items()):
        flag = 0x10 if k % 4 == 1 else 0
        if k % 7 == 3:
            planes[name] = None; records.append(bw.record_bytes(name, read.decode().upper(), flag))
            continue
        groups = mods_cases.dense_groups(rng, read)
        mismatch = k == 11
        planes[name] = None if mismatch else mods_ref.plane(read, groups)
        records.append(bw.record_bytes(name, read.decode().upper(), flag, tags=b"XYZhello\0" + tags_of(groups, k % 3 == 0, len(read) + (1 if mismatch else 0) if k % 2 else None) + b"ZZc\x05"))
    bam = str(d / "r.bam")
    bw.write_bgzf(bam, bw.header_bytes() + b"".join(records))
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", fasta, "-q", bam, "-o", prefix]
    runs, out = {}, {}
    for tag, extra, env in (("paf", ["--paf"], None), ("mods", ["--paf", "--mods", LIST], None), ("all", ["--all", "--paf", "--mods", LIST], None),
                            ("two", ["--mods", LIST, "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"}), ("merges", ["--mods", LIST], {"MM_MODS_MERGE_PAIRS": "50"}),
                            ("bam_pileup", ["--bam", "--pileup"], None), ("bam_pileup_mods", ["--bam", "--pileup", "--mods", LIST], None),
                            ("strict", ["--paf", "--mods", LIST, "--mod-min-ml", "128", "--mod-min-coverage", "2", "--min-base-quality", "20", "--pileup"], None)):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag], out[tag] = _take(prefix), p.stdout.decode()
    return dict(db=db, reads=reads, cname=cname, contigs=contigs, planes=planes, runs=runs, out=out, fasta=fasta, fastq=rd["path"], bam=bam, dir=d, n_tagged=sum(p is not None for p in planes.values()))


def _expected(world, run, min_ml=204, min_coverage=1):
    jobs = [dict(j, plane=world["planes"][name]) for j, name in _jobs_named(world, run) if j["use"]]
    rows = mods_ref.rows(mods_ref.table(jobs, min_ml), world["contigs"], CODE_BASE, min_coverage)
    return mods_ref.bedmethyl_text(rows, world["cname"], CODE_NAME), rows


def _jobs_named(world, run):
    """test_gpu_cli_pileup's jobs with their reads' names: one per ALIGNED line of PREFIX, in that order"""
    jobs = _jobs(world, run)
    names = [m.split(" ")[0] for m, e in zip(run[""].decode().splitlines(), run[".editDistances"].decode().splitlines()) if e.split(" ")[3] != "NA"]
    assert len(names) == len(jobs) and all(world["reads"][n] == j["read"] for n, j in zip(names, jobs))
    return list(zip(jobs, names))


def test_the_file_equals_the_restatement(world):
    run = world["runs"]["mods"]
    want, rows = _expected(world, run)
    assert run[".bedmethyl"] == want and len(rows) > 20000
    assert {k for _, _, _, k, *_ in rows} == {0, 1, 2} and {s for _, _, s, *_ in rows} == {1, -1}   # all three codes, both strands
    assert any(r[4] for r in rows) and any(r[5] for r in rows) and any(r[6] for r in rows) and any(r[7] for r in rows)
    cols = run[".bedmethyl"].decode().splitlines()[0].split("\t")
    assert len(cols) == 18 and cols[8] == "255,0,0" and cols[14] == cols[16] == cols[17] == "0" and cols[4] == cols[9] and int(cols[2]) == int(cols[1]) + 1
    # every other file is the file of the run without the flag
    plain = world["runs"]["paf"]
    assert set(run) == set(plain) | {".bedmethyl"}
    for suf in plain:
        assert run[suf] == plain[suf], suf
    assert "INFO, --mods: %s: 150 reads, %d with MM/ML tags; dropped: 0 groups of strand -, 0 groups of base N, 1 reads whose MN" % (world["bam"], world["n_tagged"]) in world["out"]["mods"]


def test_all_mappings_count_a_read_once(world):
    run = world["runs"]["all"]
    assert run[".bedmethyl"] == _expected(world, run)[0] and len(run[""]) >= len(world["runs"]["mods"][""])


def test_devices_batches_and_merges_do_not_change_a_byte(world):
    want = world["runs"]["mods"][".bedmethyl"]
    for tag in ("two", "merges", "bam_pileup_mods"):
        assert world["runs"][tag][".bedmethyl"] == want, tag
    a, b = world["runs"]["bam_pileup"], world["runs"]["bam_pileup_mods"]
    assert set(b) == set(a) | {".bedmethyl"}
    for suf in a:
        assert a[suf] == b[suf], suf


def test_thresholds_and_the_base_quality_floor(world):
    run = world["runs"]["strict"]
    want, rows = _expected(world, run, 128, 2)
    assert run[".bedmethyl"] == want and 0 < len(rows) < len(_expected(world, run)[1])   # (--min-base-quality does not touch the modification counts)


def test_a_fastq_query_gives_an_empty_file_and_says_why(world):
    prefix = str(world["dir"] / "fq")
    p = _run(["mapDirectly", "-r", world["fasta"], "-q", world["fastq"], "-o", prefix, "--mods", LIST])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = _take(prefix)
    assert got[".bedmethyl"] == b"" and len(got[""]) > 1000
    assert ("INFO, --mods: %s is not a BAM file and carries no MM/ML tags: its bedMethyl file is empty" % world["fastq"]) in p.stdout.decode()


def test_a_malformed_tag_ends_the_run_with_the_reads_name(world):
    name, read = next(iter(world["reads"].items()))
    bam = str(world["dir"] / "bad.bam")
    for tags, what in ((b"MMZC+m?,1,x;\0MLBC" + struct.pack("<I", 1) + b"\x05", "malformed MM tag"), (b"MMZC+m?,1;\0MLBC" + struct.pack("<I", 2) + b"\x05\x06", "ML tag holds 2 bytes")):
        bw.write_bgzf(bam, bw.header_bytes() + bw.record_bytes("fine", read.decode().upper(), 0) + bw.record_bytes(name, read.decode().upper(), 0, tags=tags))
        p = _run(["mapDirectly", "-r", world["fasta"], "-q", bam, "-o", str(world["dir"] / "bad"), "--mods", LIST])
        err = p.stderr.decode()
        assert p.returncode == 1 and bam in err and "read " + name + ":" in err and what in err, err[-1000:]
        _take(str(world["dir"] / "bad"))


def test_refusals_name_the_flag(world, tmp_path):
    base = ["-r", world["fasta"], "-q", world["bam"], "-o", str(tmp_path / "o")]
    for mode, extra, what in (("mapDirectly", ["--mods", LIST, "--hpc"], "--mods cannot be combined with --hpc"),
                              ("mapDirectly", ["--mods", LIST, "--shard-index"], "--mods cannot be combined with --shard-index or --stream-chunks"),
                              ("mapDirectly", ["--mods", LIST, "--stream-chunks"], "--mods cannot be combined with --shard-index or --stream-chunks"),
                              ("mapAgainstIndex", ["--mods", LIST], "--mods belongs to mapDirectly"),
                              ("mapDirectly", ["--mods", "C+m,C+m"], "--mods: the item C+m is given twice"),
                              ("mapDirectly", ["--mods", "C+m,C+h,A+a,T+g,G+x"], "--mods takes 1 to 4"),
                              ("mapDirectly", ["--mods", "N+m"], "--mods takes 1 to 4"),
                              ("mapDirectly", ["--mods", LIST, "--mod-min-ml", "256"], "--mods: --mod-min-ml takes an integer from 0 to 255"),
                              ("mapDirectly", ["--mods", LIST, "--mod-min-coverage", "0"], "--mods: --mod-min-coverage takes an integer from 1"),
                              ("mapDirectly", ["--mod-min-ml", "9"], "--mod-min-ml needs --mods"),
                              ("mapDirectly", ["--mod-min-coverage", "9"], "--mod-min-coverage needs --mods")):
        p = _run([mode] + base + extra)
        assert p.returncode == 1 and what in p.stderr.decode(), (extra, p.stderr.decode()[-500:])
        assert _take(str(tmp_path / "o")) == {}                     # before any work
