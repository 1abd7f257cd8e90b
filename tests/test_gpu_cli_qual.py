"""`mapDirectly --base-qualities` and `--min-base-quality Q` on the world of tests/test_gpu_cli_pileup.py (2 genomes of 30 kb, 150 reads of 2 kb), whose FASTQ is
rewritten with per-base qualities drawn in 2 .. 40 from a fixed seed, independent of the bases.  PREFIX.bam carries the reads' qualities and is otherwise the
file of the run without the flag; under a floor of 20 PREFIX.pileup, .vcf and .consensus.* equal what tests/qual_ref.py computes from the run's own PREFIX,
.editDistances and .paf with the qualities, and every other file stays byte for byte.  The same files come out of the reads as bgzip'd FASTQ, as plain gzip, as
unaligned BAM (upper-cased, as BAM holds bases; half the records reverse-complemented) and from two logical devices in batches of 5 reads; a FASTA query under the flag gives the BAM of the run
without it; the refusals name their flag."""
import glob
import gzip
import struct

import numpy as np
import pytest

import bam_writer
import cons_ref
import pileup_ref
import qual_ref
import vcf_ref
from test_gpu_cli_edit_distance import SAME, _run, _take
from test_gpu_cli_pileup import _jobs

pytestmark = pytest.mark.gpu

FLOOR = 20
QUAL_SEED = 20                                                    # (fixed; 18 of the 39 values drawn lie under the floor: test_not_vacuous holds the share dropped)
OUT = ["--paf", "--bam", "--pileup", "--pileup-min-count", "1", "--pileup-min-frac", "0", "--vcf", "--vcf-min-count", "1", "--vcf-min-frac", "0", "--consensus"]
UNTOUCHED = SAME + (".editDistances", ".paf", ".pileup.contigs")


def qual_record_bytes(name, read, qual, flag):
    """bam_writer.record_bytes with the read's qualities in place of the 0xFF bytes: stored reversed where the read is stored reverse-complemented"""
    plain = bam_writer.record_bytes(name, read, flag)
    stored = bytes(qual[::-1] if flag & 0x10 else qual)
    assert plain.endswith(b"\xff" * len(read)) and len(stored) == len(read)
    return plain[:len(plain) - len(read)] + stored


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("qualcli")
    db = synth.make_db(str(d / "db"), n_genomes=2, genome_len=30_000, seed=11, contigs_per_genome=1, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r0.fq"), n_reads=150, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    order = [lines[i][1:].split()[0].decode() for i in range(0, len(lines) - 1, 4)]
    reads = {n: lines[4 * k + 1] for k, n in enumerate(order)}
    rng = np.random.default_rng(QUAL_SEED)
    quals = {n: rng.integers(2, 41, size=len(reads[n])).astype(np.uint8).tobytes() for n in order}
    fq, fa = str(d / "r.fq"), str(d / "r.fa")
    text = b"".join(b"@" + n.encode() + b"\n" + reads[n] + b"\n+\n" + bytes(b + 33 for b in quals[n]) + b"\n" for n in order)
    open(fq, "wb").write(text)
    open(fa, "wb").write(b"".join(b">" + n.encode() + b"\n" + reads[n] + b"\n" for n in order))
    bgz, gz, ubam = str(d / "rz.fq.gz"), str(d / "rg.fq.gz"), str(d / "r.bam")
    bam_writer.write_bgzf(bgz, text, 7777)
    open(gz, "wb").write(gzip.compress(text, 6))
    bam_writer.write_bgzf(ubam, bam_writer.header_bytes() + b"".join(qual_record_bytes(n, reads[n].decode().upper(), quals[n], 0x10 if k % 2 else 0) for k, n in enumerate(order)), 20000)
    even = [c for g in range(0, len(db.genome_contigs), 2) for c in db.genome_contigs[g]]
    cname, contigs = [db.contig_ids[c].split()[0] for c in even], [db.contig_seqs[c].tobytes() for c in even]
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for c in even:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    prefix = str(d / "out")
    floor = ["--min-base-quality", str(FLOOR)]
    runs, said = {}, {}
    for tag, q, extra, env in (("plain", fq, OUT, None), ("bq", fq, OUT + ["--base-qualities"], None), ("floor", fq, OUT + floor, None),
                               ("bgzip", bgz, OUT + floor, None), ("gzip", gz, OUT + floor, None), ("ubam", ubam, OUT + floor, None),
                               ("two", fq, OUT + floor + ["--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"}),
                               ("fasta", fa, ["--bam"], None), ("fasta_bq", fa, ["--bam", "--base-qualities"], None)):
        p = _run(["mapDirectly", "-r", fasta, "-q", q, "-o", prefix] + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag], said[tag] = _take(prefix), p.stdout.decode()
    return dict(db=db, reads=reads, quals=quals, cname=cname, contigs=contigs, runs=runs, said=said, fasta=fasta, q=fq)


def jobs_of(world, run):
    """the primary aligned records of a run as qual_ref's jobs: test_gpu_cli_pileup's, from the run's own files, with the reads' qualities"""
    maps = [m.split(" ") for m, e in zip(run[""].decode().splitlines(), run[".editDistances"].decode().splitlines()) if e.split(" ")[3] != "NA"]
    jobs = _jobs(world, run)
    assert len(maps) == len(jobs)
    return [dict(j, qual=world["quals"][m[0]]) for j, m in zip(jobs, maps) if j["use"]]


def bam_records(data):
    """(the inflated stream with every QUAL blanked, [(name, flag, QUAL)]) of a BAM file"""
    raw = bytearray(gzip.decompress(data))
    assert raw[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    recs = []
    while at < len(raw):
        size, = struct.unpack_from("<i", raw, at)
        l_name, n_cig, flag, l_seq = raw[at + 12], struct.unpack_from("<H", raw, at + 16)[0], struct.unpack_from("<H", raw, at + 18)[0], struct.unpack_from("<i", raw, at + 20)[0]
        q = at + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        recs.append((bytes(raw[at + 36:at + 36 + l_name - 1]).decode(), flag, bytes(raw[q:q + l_seq])))
        raw[q:q + l_seq] = b"\xff" * l_seq
        at += 4 + size
    assert at == len(raw)
    return bytes(raw), recs


def test_every_other_file_stays_byte_for_byte(world):
    plain, bq, floor = (world["runs"][t] for t in ("plain", "bq", "floor"))
    assert set(plain) == set(bq) == set(floor) and set(plain) >= set(UNTOUCHED) | {".bam", ".pileup", ".vcf", ".consensus.fa", ".consensus.tsv"}
    for suf in UNTOUCHED:
        assert plain[suf] == bq[suf] == floor[suf], suf
    for suf in (".pileup", ".vcf", ".consensus.fa", ".consensus.tsv"):      # --base-qualities alone changes the BAM and nothing else
        assert plain[suf] == bq[suf], suf
    assert bq[".bam"] == floor[".bam"] != plain[".bam"]


def test_bam_carries_the_qualities(world):
    blank_p, recs_p = bam_records(world["runs"]["plain"][".bam"])
    blank_q, recs_q = bam_records(world["runs"]["bq"][".bam"])
    assert blank_q == blank_p and len(recs_q) == len(recs_p) > 100
    assert {f & 0x10 for _, f, _ in recs_q} == {0, 0x10}
    for (name, flag, qual), (_, _, none) in zip(recs_q, recs_p):
        want = qual_ref.bam_qual(dict(read=world["reads"][name], qual=world["quals"][name], strand=-1 if flag & 0x10 else 1))
        assert qual == want and none == b"\xff" * len(want), name


def test_not_vacuous(world):
    """qual_ref alone drops between 20 % and 80 % of this world's events at the floor; the filtered pileup is a proper, non-empty part of the unfiltered one"""
    jobs = jobs_of(world, world["runs"]["floor"])
    full, kept = sum(qual_ref.table(jobs, 0).values()), sum(qual_ref.table(jobs, FLOOR).values())
    print(f"events without a floor {full}, kept at {FLOOR}: {kept} ({100 * (full - kept) / full:.1f} % dropped)")
    assert full > 2000 and 0.2 * full < full - kept < 0.8 * full, (full, kept)
    sites = lambda run: {tuple(ln.split("\t")[:4]): int(ln.split("\t")[4]) for ln in run[".pileup"].decode().splitlines()}
    a, b = sites(world["runs"]["plain"]), sites(world["runs"]["floor"])
    assert 0 < len(b) < len(a) and set(b) < set(a) and all(b[k] <= a[k] for k in b)


def test_pileup_vcf_and_consensus_equal_the_restatement(world):
    run, plain = world["runs"]["floor"], world["runs"]["plain"]
    jobs = jobs_of(world, run)
    clen, cname, contigs = [len(c) for c in world["contigs"]], world["cname"], world["contigs"]
    iv = [pileup_ref.interval(j) for j in jobs]
    sites, _ = pileup_ref.finish(qual_ref.table(jobs, FLOOR), iv, clen, 1, 0.0)
    assert run[".pileup"] == pileup_ref.pileup_text(sites, cname, [c.upper() for c in contigs])
    t = qual_ref.vcf_table(jobs, contigs, FLOOR)
    head = "##source=metamaps mapDirectly --vcf\n"
    want = vcf_ref.vcf_text(vcf_ref.finish(t, iv, contigs, 1, 0.0), cname, clen).decode().replace(head, head + f"##minBaseQuality={FLOOR}\n")
    assert run[".vcf"].decode() == want
    # aside from that one line the file has the shape of the unfiltered one: the same header, fewer lines of the same eight columns
    mine, theirs = run[".vcf"].decode().splitlines(), plain[".vcf"].decode().splitlines()
    assert [ln for ln in mine if ln.startswith("#") and "minBaseQuality" not in ln] == [ln for ln in theirs if ln.startswith("#")]
    body = [ln for ln in mine if not ln.startswith("#")]
    assert 0 < len(body) < len([ln for ln in theirs if not ln.startswith("#")]) and all(len(ln.split("\t")) == 8 for ln in body) and set(body) - set(theirs) != set(body)
    res = cons_ref.consensus(t, iv, contigs, 3, 0.5, 0.0)
    assert run[".consensus.fa"] == cons_ref.fasta_text(res, cname) and run[".consensus.tsv"] == cons_ref.tsv_text(res, cname, clen)
    assert "minBaseQuality" not in plain[".vcf"].decode() and "minBaseQuality" not in world["runs"]["bq"][".vcf"].decode()


@pytest.mark.parametrize("tag", ["bgzip", "gzip", "ubam", "two"])
def test_the_same_files_from_every_kind_of_source(world, tag):
    a, b = world["runs"]["floor"], world["runs"][tag]
    assert set(a) == set(b)
    for suf in sorted(a):
        if suf == ".parameters" and tag != "two":                   # (names its query file; every other line is the same)
            diff = [(x, y) for x, y in zip(a[suf].split(b"\n"), b[suf].split(b"\n")) if x != y]
            assert len(diff) == 1 and b"r.fq" in diff[0][0], (tag, diff)
        elif suf == ".bam" and tag == "two":                        # (the members are cut per batch: the inflated stream is what stays)
            assert gzip.decompress(a[suf]) == gzip.decompress(b[suf]), (tag, suf)
        else:
            assert a[suf] == b[suf], (tag, suf)


def test_a_fasta_query_under_the_flag(world):
    assert world["runs"]["fasta_bq"] == world["runs"]["fasta"] and len(world["runs"]["fasta"][".bam"]) > 1000
    assert bam_records(world["runs"]["fasta"][".bam"])[0] == bam_records(world["runs"]["plain"][".bam"])[0]
    info = [ln for ln in world["said"]["fasta_bq"].splitlines() if "--base-qualities" in ln]
    assert len(info) == 1 and "r.fa" in info[0] and "no qualities" in info[0]
    assert not any("--base-qualities" in ln for t in ("fasta", "bq", "floor", "ubam") for ln in world["said"][t].splitlines())


def test_refusals_name_their_flag(world, tmp_path):
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["plain"][""])
    io = ["-r", fasta, "-q", q, "-o", x]
    bq, mbq = "--base-qualities", "--min-base-quality"
    for args, flag in ((["mapDirectly", bq] + io, bq), (["mapDirectly", bq, "--pileup"] + io, bq), (["mapDirectly", bq, "--paf"] + io, bq),
                       (["mapDirectly", mbq, "20"] + io, mbq), (["mapDirectly", mbq, "20", "--bam"] + io, mbq), (["mapDirectly", mbq, "20", "--paf"] + io, mbq),
                       (["mapDirectly", "--pileup", mbq, "94"] + io, mbq), (["mapDirectly", "--vcf", mbq, "-1"] + io, mbq), (["mapDirectly", "--consensus", mbq, "x"] + io, mbq),
                       (["index", bq, "--bam", "-r", fasta, "-i", x], bq), (["mapAgainstIndex", "--pileup", mbq, "20", "-i", x, "-q", q, "-o", x], mbq),
                       (["classify", bq, "--bam", "--DB", db.dir, "--mappings", maps], bq), (["classify", "--vcf", mbq, "20", "--DB", db.dir, "--mappings", maps], mbq),
                       (["mapDirectly", "--hpc", "--bam", bq] + io, bq), (["mapDirectly", "--hpc", "--pileup", mbq, "20"] + io, mbq),
                       (["mapDirectly", "--shard-index", "--bam", bq] + io, bq), (["mapDirectly", "--stream-chunks", "--vcf", mbq, "20"] + io, mbq)):
        p = _run(args)
        err = p.stderr.decode()
        assert p.returncode == 1 and err.startswith(flag + " "), (args, err[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
