"""`mapDirectly --error-profile`: PREFIX.errorProfile.substitutions, .indels, .qualities and .contigs beside outputs that stay byte for byte, on a synthetic
reference of four contigs and 200 reads of 2 kb whose FASTQ carries per-base qualities drawn from a fixed seed.  The four files equal what tests/errprof_ref.py
computes from the same run's PREFIX (field 14 gives a read's primary record), .editDistances, .paf (the cg runs), the reads, their qualities and the reference;
the same files come from batches of 7 reads on two logical devices, from the reads as unaligned BAM and beside other side outputs; without --base-qualities only
the row `none` appears; an empty run writes the headers alone; the refusals name the flag, and --base-qualities alone stays refused."""
import glob

import numpy as np
import pytest

import bam_writer
import errprof_ref
from test_gpu_cli_edit_distance import SAME, _run, _take
from test_gpu_cli_pileup import _jobs
from test_gpu_cli_qual import qual_record_bytes

pytestmark = pytest.mark.gpu
OURS = (".errorProfile.substitutions", ".errorProfile.indels", ".errorProfile.qualities", ".errorProfile.contigs")
FLAG = "--error-profile"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("errprofcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11, contigs_per_genome=2, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r0.fq"), n_reads=200, read_len=2000, seed=5)
    lines = open(rd["path"], "rb").read().split(b"\n")
    order = [lines[i][1:].split()[0].decode() for i in range(0, len(lines) - 1, 4)]
    reads = {n: lines[4 * k + 1].upper() for k, n in enumerate(order)}   # (upper case, as BAM holds bases: one set of reads for both sources)
    rng = np.random.default_rng(31)
    quals = {n: rng.integers(0, 94, size=len(reads[n])).astype(np.uint8).tobytes() for n in order}
    fq, ubam = str(d / "r.fq"), str(d / "r.bam")
    open(fq, "wb").write(b"".join(b"@" + n.encode() + b"\n" + reads[n] + b"\n+\n" + bytes(b + 33 for b in quals[n]) + b"\n" for n in order))
    bam_writer.write_bgzf(ubam, bam_writer.header_bytes() + b"".join(qual_record_bytes(n, reads[n].decode(), quals[n], 0x10 if k % 2 else 0) for k, n in enumerate(order)), 20000)
    even = [c for g in range(0, len(db.genome_contigs), 2) for c in db.genome_contigs[g]]
    cname, contigs = [db.contig_ids[c].split()[0] for c in even], [db.contig_seqs[c].tobytes() for c in even]
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for c in even:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    prefix = str(d / "out")
    bq = "--base-qualities"
    others = ["--bam", "--pileup", "--vcf", "--depth", "--consensus"]
    runs, said = {}, {}
    for tag, q, extra, env in (("paf", fq, ["--paf"], None), ("profile", fq, [FLAG, "--paf", bq], None),
                               ("batch7", fq, [FLAG, bq, "--devices", "0,0"], {"MM_CLI_BATCH_READS": "7"}), ("ubam", ubam, [FLAG, bq], None),
                               ("others", fq, others + [bq], None), ("with_others", fq, [FLAG] + others + [bq], None), ("no_qualities", fq, [FLAG], None),
                               ("empty", fq, [FLAG, bq, "-m", "5000"], None), ("compress", fq, [FLAG, bq, "--compress-output"], None)):
        p = _run(["mapDirectly", "-r", fasta, "-q", q, "-o", prefix] + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag], said[tag] = _take(prefix), p.stdout.decode()
    return dict(db=db, reads=reads, quals=quals, cname=cname, contigs=contigs, runs=runs, said=said, fasta=fasta, q=fq)


def expected(world, run, with_qualities=True):
    """the four texts of the restatement from the run's own PREFIX, .editDistances and .paf"""
    maps = [m.split(" ") for m, e in zip(run[""].decode().splitlines(), run[".editDistances"].decode().splitlines()) if e.split(" ")[3] != "NA"]
    jobs = _jobs(world, run)
    assert len(maps) == len(jobs)
    jobs = [dict(j, qual=list(world["quals"][m[0]]) if with_qualities else None) for j, m in zip(jobs, maps)]
    counters, cols, keys = errprof_ref.profile(jobs, world["contigs"])
    t = errprof_ref.unflat(counters)
    listed, rows, total = errprof_ref.finish(keys, cols)
    clen = [len(c) for c in world["contigs"]]
    texts = (errprof_ref.substitutions_text(t), errprof_ref.indels_text(t), errprof_ref.qualities_text(t), errprof_ref.contigs_text(listed, rows, total, world["cname"], clen))
    return dict(zip(OURS, texts)), t, (listed, rows, total), jobs


def test_the_four_files_equal_the_restatement(world):
    run = world["runs"]["profile"]
    want, t, (listed, rows, total), jobs = expected(world, run)
    for suf in OURS:
        assert run[suf].decode() == want[suf], suf
    # the world is not degenerate
    used = [j for j in jobs if j["use"]]
    assert len(used) >= 100 and {j["strand"] for j in used} == {1, -1} and len(listed) >= 2 and total[0] == len(used)
    assert sum(t["sub"][a][a] for a in range(4)) > 100_000 and all(t["sub"][a][b] > 0 for a in range(4) for b in range(4))
    assert all(sum(t["indel"][k][h]) > 0 for k in range(2) for h in range(2)) and sum(1 for q in range(94) if t["qual"][0][q]) == 94 and sum(t["qual"][s][94] for s in range(3)) == 0
    assert len(run[".errorProfile.qualities"].splitlines()) == 95 and run[".errorProfile.contigs"].decode().splitlines()[-1].startswith("*\t")
    assert total[7] < total[9] < total[11]                          # the identities of the reads spread


def test_every_other_file_is_the_file_of_the_run_without_the_flag(world):
    a, b = world["runs"]["paf"], world["runs"]["profile"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    a, b = world["runs"]["others"], world["runs"]["with_others"]      # beside every other side output, which share the one alignment call
    assert set(b) == set(a) | set(OURS) and len(a) >= 14
    for suf in a:
        assert a[suf] == b[suf], suf


@pytest.mark.parametrize("tag", ["batch7", "ubam", "with_others", "compress"])
def test_the_same_four_files_from_other_batches_sources_and_flags(world, tag):
    a, b = world["runs"]["profile"], world["runs"][tag]
    for suf in OURS:
        assert b[suf] == a[suf], (tag, suf)
    if tag == "compress":
        assert ".gz" in b


def test_without_base_qualities_only_the_none_row(world):
    run = world["runs"]["no_qualities"]
    want, t, _, _ = expected(world, dict(run, **{".paf": world["runs"]["profile"][".paf"]}), with_qualities=False)
    for suf in OURS:
        assert run[suf].decode() == want[suf], suf
    lines = run[".errorProfile.qualities"].decode().splitlines()
    assert len(lines) == 2 and lines[1].startswith("none\t")
    for suf in OURS[:2] + OURS[3:]:                                   # the qualities touch nothing else
        assert run[suf] == world["runs"]["profile"][suf], suf
    info = [ln for ln in world["said"]["no_qualities"].splitlines() if ln.startswith("INFO, --error-profile")]
    assert len(info) == 1 and "carried a base quality" in info[0]
    assert not any(ln.startswith("INFO, --error-profile") for t in ("profile", "ubam", "batch7", "empty") for ln in world["said"][t].splitlines())


def test_an_empty_run_writes_the_headers_alone(world):
    run = world["runs"]["empty"]                                    # no read is as long as -m asks
    assert run.get("", b"") == b""
    assert [run[suf].decode() for suf in OURS] == [errprof_ref.SUB_HEADER, errprof_ref.INDEL_HEADER, errprof_ref.QUAL_HEADER, errprof_ref.CONTIGS_HEADER]


def test_refused_combinations(world, tmp_path):
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["paf"][""])
    io = ["-r", fasta, "-q", q, "-o", x]
    for args, flag in ((["mapDirectly", FLAG, "--hpc"] + io, FLAG), (["mapDirectly", FLAG, "--shard-index"] + io, FLAG), (["mapDirectly", FLAG, "--stream-chunks"] + io, FLAG),
                       (["mapDirectly", FLAG, "--depth", "--pileup", "--hpc"] + io, FLAG), (["mapAgainstIndex", FLAG, "-i", x, "-q", q, "-o", x], FLAG),
                       (["index", FLAG, "-r", fasta, "-i", x], FLAG), (["classify", FLAG, "--DB", db.dir, "--mappings", maps], FLAG),
                       (["mapDirectly", "--base-qualities"] + io, "--base-qualities"), (["mapDirectly", "--base-qualities", "--paf"] + io, "--base-qualities"),
                       (["mapDirectly", "--base-qualities", FLAG, "--hpc"] + io, "--base-qualities")):
        p = _run(args)
        err = p.stderr.decode()
        assert p.returncode == 1 and err.startswith(flag + " "), (args, err[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
    assert _run(["mapDirectly", "--base-qualities"] + io).stderr.decode().startswith("--base-qualities needs --bam or --min-base-quality")
