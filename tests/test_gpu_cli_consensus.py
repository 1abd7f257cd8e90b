"""`mapDirectly --consensus`: PREFIX.consensus.fa and PREFIX.consensus.tsv beside outputs that stay byte for byte, on the world of tests/test_gpu_cli_vcf.py
(one contig of 30 kb with a homopolymer of 12, a dinucleotide repeat and a homopolymer of 300; reads from a strain copy with planted substitutions, deletions
and insertions, with light noise).  Both files equal what tests/cons_ref.py computes from the same run's PREFIX, .editDistances and .paf; the same bytes come
out under --all --then-classify, from two logical devices in small batches, with the accumulator merged every 50 triples, with one base per group and together
with --vcf --pileup --bam --compress-output; PREFIX.vcf is --vcf's own; the refused combinations name --consensus.  The planted truth itself, through
perfect alignments, gives the strain back: a CPU test."""
import glob

import numpy as np
import pytest

import cons_ref
import vcf_ref
from test_gpu_cli_vcf import READ_LEN, SEED, planted, read_spans, truth_jobs

OURS = (".consensus.fa", ".consensus.tsv")


def test_the_planted_truth_gives_the_strain_back():
    ref, strain, segs, edits = planted()
    jobs = truth_jobs(ref, strain, segs, read_spans())
    iv = [vcf_ref.interval(j) for j in jobs]
    s, text, col = cons_ref.consensus(vcf_ref.table(jobs, [ref]), iv, [ref], 3, 0.5, 0.0)[0]
    assert (s["snvs"], s["deletions"], s["insertions"], s["dropped"]) == (29, 6, 3, 0)
    shallow = [pos for pos, (kind, _) in edits.items() if kind == "X" and vcf_ref.depth(iv, 0, pos) < 3]
    assert sum(1 for kind, _ in edits.values() if kind == "X") == 30 and len(shallow) == 1      # the 30th SNV lies under depth 3
    assert s["consensusLength"] == len(text) == 29_997 == len(strain)
    assert len(ref) - s["called"] == 1_406
    assert all(a == "N" or a == chr(b) for a, b in zip(text, strain))
    assert text.count("N") < 1_500 and s["written"] == 1


def build_world(d):
    """the reference, the noisy reads of the vcf test's world and every run of the command line, in the directory d"""
    from metamaps_amd import synth
    from test_gpu_cli_edit_distance import _run, _take
    ref, strain, segs, edits = planted()
    rng = np.random.default_rng(SEED + 2)
    db = synth.write_db_dir(str(d / "db"), [(0, ref), (1, synth.random_genome(rng, 30_000).tobytes())])
    cname = [open(db["fasta"], "rb").readline()[1:].split()[0].decode()]
    fasta, q = str(d / "ref.fa"), str(d / "r.fq")
    open(fasta, "wb").write(b">" + cname[0].encode() + b"\n" + ref + b"\n")
    reads = {}
    with open(q, "wb") as f:
        for k, (s0, strand) in enumerate(read_spans()):
            s = np.frombuffer(strain[s0:s0 + READ_LEN], dtype=np.uint8).copy()
            s = synth.mutate(rng, synth.revcomp(s) if strand < 0 else s, 0.006, 0.002, 0.002)
            reads[f"read{k:04d}"] = s.tobytes()
            f.write(b"@read%04d\n" % k + s.tobytes() + b"\n+\n" + b"I" * s.size + b"\n")
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", fasta, "-q", q, "-o", prefix]
    classify = ["--all", "--then-classify", db["dir"], "--minreads", "3"]
    rest = ["--vcf", "--pileup", "--bam", "--compress-output"]
    runs = {}
    for tag, extra, env in (("paf", ["--paf"], None), ("cons", ["--paf", "--consensus"], None),
                            ("all_paf", classify + ["--paf"], None), ("all", classify + ["--paf", "--consensus"], None),
                            ("two", ["--consensus", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "5"}),
                            ("merges", ["--consensus"], {"MM_VCF_MERGE_PAIRS": "50"}), ("groups", ["--consensus"], {"MM_CONS_GROUP_BASES": "1"}),
                            ("vcf", ["--vcf"], None), ("cons_vcf", ["--consensus", "--vcf"], None),
                            ("rest", rest, None), ("combo", rest + ["--consensus"], None),
                            ("strict", ["--consensus", "--consensus-min-depth", "10", "--consensus-min-frac", "0.9", "--consensus-min-called", "0.99"], None),
                            ("empty", ["--consensus", "-m", "5000"], None)):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, cname=cname, contigs=[ref], edits=edits, runs=runs, fasta=fasta, q=q)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return build_world(tmp_path_factory.mktemp("conscli"))


def _expected(world, run, min_depth=3, min_frac=0.5, min_called=0.0):
    from test_gpu_cli_pileup import _jobs
    jobs = [j for j in _jobs(world, run) if j["use"]]
    iv = [vcf_ref.interval(j) for j in jobs]
    res = cons_ref.consensus(vcf_ref.table(jobs, world["contigs"]), iv, world["contigs"], min_depth, min_frac, min_called)
    return cons_ref.fasta_text(res, world["cname"]), cons_ref.tsv_text(res, world["cname"], [len(c) for c in world["contigs"]]), res, iv


@pytest.mark.gpu
def test_both_files_equal_the_restatement(world):
    run = world["runs"]["cons"]
    fa, tsv, res, iv = _expected(world, run)
    assert run[".consensus.fa"] == fa and run[".consensus.tsv"] == tsv and len(iv) >= 150
    # non-degeneracy: every planted SNV at depth >= 10 is in the consensus at its mapped column; the indels are there; lines are 60 columns
    s, text, col = res[0]
    deep = [pos for pos, (kind, _) in world["edits"].items() if kind == "X" and vcf_ref.depth(iv, 0, pos) >= 10]
    assert len(deep) >= 10 and all(text[col[pos]] == world["edits"][pos][1].decode() for pos in deep)
    lines = run[".consensus.fa"].decode().splitlines()
    assert lines[0] == ">" + world["cname"][0] and all(len(ln) == 60 for ln in lines[1:-1]) and 1 <= len(lines[-1]) <= 60 and "".join(lines[1:]) == text
    row = dict(zip(cons_ref.TSV_HEADER.split(), run[".consensus.tsv"].decode().splitlines()[1].split("\t")))
    assert int(row["deletions"]) >= 5 and int(row["insertions"]) == 3 and int(row["snvs"]) >= 25 and row["written"] == "1" and int(row["consensusLength"]) == len(text)
    assert run[".consensus.tsv"].decode().splitlines()[0] + "\n" == cons_ref.TSV_HEADER and len(run[".consensus.tsv"].splitlines()) == 2
    assert ".vcf" not in run and ".editDistances" in run            # --consensus implies --edit-distance and writes no .vcf


@pytest.mark.gpu
def test_the_thresholds(world):
    run = world["runs"]["strict"]
    fa, tsv, res, _ = _expected(world, world["runs"]["cons"], 10, 0.9, 0.99)
    assert run[".consensus.fa"] == fa and run[".consensus.tsv"] == tsv
    assert res[0][0]["written"] == 0 and fa == b"" and 0 < res[0][0]["called"] < 29_700 and res[0][0]["consensusLength"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["all", "two", "merges", "groups", "cons_vcf", "combo"])
def test_the_same_bytes_in_every_variant(world, tag):
    a, b = world["runs"]["cons"], world["runs"][tag]
    for suf in OURS:
        assert b[suf] == a[suf], (tag, suf)
    if tag == "all":                                                # a read with several records counts once: the restatement on this run's own files
        fa, tsv, _, _ = _expected(world, b)
        assert (b[".consensus.fa"], b[".consensus.tsv"]) == (fa, tsv)
    if tag == "combo":
        assert len(b[".bam"]) > 1000 and not b[".consensus.fa"].startswith(b"\x1f\x8b") and b[".consensus.tsv"].startswith(b"contigID\t")   # plain text under --compress-output


@pytest.mark.gpu
def test_the_vcf_is_the_vcf_of_the_run_without_the_flag(world):
    runs = world["runs"]
    assert runs["cons_vcf"][".vcf"] == runs["vcf"][".vcf"] and len(runs["vcf"][".vcf"].splitlines()) > 40
    assert set(runs["cons_vcf"]) == set(runs["vcf"]) | set(OURS)
    for tag in ("cons", "two", "merges", "groups", "all"):
        assert ".vcf" not in runs[tag], tag
    assert runs["combo"][".vcf"] == runs["rest"][".vcf"]


@pytest.mark.gpu
def test_every_other_file_is_the_file_of_the_run_without_the_flag(world):
    from test_gpu_cli import CLASSIFY_SUFFIXES
    from test_gpu_cli_edit_distance import SAME
    a, b = world["runs"]["paf"], world["runs"]["cons"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    a, b = world["runs"]["all_paf"], world["runs"]["all"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + CLASSIFY_SUFFIXES + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    assert len(a[".EM.WIMP"]) > 100
    a, b = world["runs"]["rest"], world["runs"]["combo"]
    assert ".gz" in b and set(b) == set(a) | set(OURS)
    for suf in a:
        assert a[suf] == b[suf], suf


@pytest.mark.gpu
def test_an_empty_run_writes_an_empty_fasta_and_the_header_alone(world):
    run = world["runs"]["empty"]                                    # no read is as long as -m asks
    assert run[".consensus.fa"] == b"" and run[".consensus.tsv"] == cons_ref.TSV_HEADER.encode() and run.get("", b"") == b""


@pytest.mark.gpu
def test_refused_combinations(world, tmp_path):
    from test_gpu_cli_edit_distance import _run
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["paf"][""])
    io = ["-r", fasta, "-q", q, "-o", x]
    for args in (["mapDirectly", "--consensus", "--hpc"] + io,
                 ["mapDirectly", "--consensus", "--shard-index"] + io,
                 ["mapDirectly", "--consensus", "--stream-chunks", "--maxmemory-bytes", "100000"] + io,
                 ["mapDirectly", "--consensus", "--vcf", "--pileup", "--hpc"] + io,
                 ["index", "--consensus", "-r", fasta, "-i", x],
                 ["mapAgainstIndex", "--consensus", "-i", x, "-q", q, "-o", x],
                 ["classify", "--consensus", "--DB", db["dir"], "--mappings", maps],
                 ["mapDirectly", "--consensus", "--consensus-min-depth", "0"] + io,
                 ["mapDirectly", "--consensus", "--consensus-min-depth", "2.5"] + io,
                 ["mapDirectly", "--consensus", "--consensus-min-frac", "0.49"] + io,
                 ["mapDirectly", "--consensus", "--consensus-min-frac", "1.5"] + io,
                 ["mapDirectly", "--consensus", "--consensus-min-called", "1.01"] + io,
                 ["mapDirectly", "--consensus", "--consensus-min-called", "-0.5"] + io,
                 ["mapDirectly", "--consensus-min-depth", "2"] + io,
                 ["mapDirectly", "--vcf", "--consensus-min-frac", "0.5"] + io,
                 ["mapDirectly", "--pileup", "--consensus-min-called", "0.5"] + io):
        p = _run(args)
        assert p.returncode == 1 and "--consensus" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
