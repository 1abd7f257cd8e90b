"""`mapDirectly --pileup`: PREFIX.pileup and PREFIX.pileup.contigs beside outputs that stay byte for byte.  The reference holds one genome, the reads come
from it and from its 3 % substitution copy, so a third of them carry real variants.  The two files equal what tests/pileup_ref.py computes from the same
run's PREFIX (field 14 gives a read's primary record), .editDistances, .paf (the cg runs: other tests hold them to the naive walk), the reads and the
reference; the same files come out under --all, from two logical devices in small batches, with the accumulator merged every 50 pairs, and with --bam;
the refused combinations name --pileup."""
import glob
import re

import pytest

import pileup_ref
from test_gpu_cli import CLASSIFY_SUFFIXES
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu
LOOSE = ["--pileup-min-count", "1", "--pileup-min-frac", "0"]
OURS = (".pileup", ".pileup.contigs")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("pileupcli")
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
    prefix = str(d / "out")
    base = ["mapDirectly", "-r", fasta, "-q", rd["path"], "-o", prefix]
    classify = ["--all", "--then-classify", db.dir, "--minreads", "3"]
    runs = {}
    for tag, extra, env in (("paf", ["--paf"], None), ("loose", ["--paf", "--pileup"] + LOOSE, None), ("default", ["--pileup"], None),
                            ("all_paf", classify + ["--paf"], None), ("all", classify + ["--paf", "--pileup"] + LOOSE, None),
                            ("two", ["--pileup", "--devices", "0,0"] + LOOSE, {"MM_CLI_BATCH_READS": "5"}),
                            ("merges", ["--pileup"] + LOOSE, {"MM_PILEUP_MERGE_PAIRS": "50"}), ("bam", ["--bam", "--pileup"] + LOOSE, None)):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, cname=cname, contigs=contigs, runs=runs, fasta=fasta, q=rd["path"])


def _jobs(world, run):
    """pileup_ref's jobs of a run from its own files: one per ALIGNED line of PREFIX, use = 1 on the aligned line with the largest field 14 of its read"""
    maps, eds, paf = run[""].decode().splitlines(), run[".editDistances"].decode().splitlines(), iter(run[".paf"].decode().splitlines())
    assert len(maps) == len(eds)
    jobs, best = [], {}
    for m, e in zip(maps, eds):
        f, g = m.split(" "), e.split(" ")
        if g[3] == "NA":
            continue
        c = next(paf).split("\t")
        assert c[0] == f[0] == g[0] and c[5] == f[5] and c[7] == g[4]
        runs = [int(n) << 4 | {"I": 1, "D": 2, "=": 7, "X": 8}[op] for n, op in re.findall(r"(\d+)([=XID])", c[13][5:])]
        jobs.append(dict(read=world["reads"][f[0]], strand=1 if f[4] == "+" else -1, c=world["cname"].index(f[5]), first=int(g[4]), runs=runs, d=int(g[3]), use=0))
        assert pileup_ref.interval(jobs[-1])[2] == int(g[5])
        if f[0] not in best or float(f[13]) > best[f[0]][0]:       # the first of equals stays
            best[f[0]] = (float(f[13]), len(jobs) - 1)
    assert next(paf, None) is None
    for _, k in best.values():
        jobs[k]["use"] = 1
    return jobs


def _expected(world, run, min_count, min_frac):
    jobs = [j for j in _jobs(world, run) if j["use"]]
    clen = [len(c) for c in world["contigs"]]
    sites, contigs = pileup_ref.finish(pileup_ref.table(jobs), [pileup_ref.interval(j) for j in jobs], clen, min_count, min_frac)
    upper = [c.upper() for c in world["contigs"]]
    return pileup_ref.pileup_text(sites, world["cname"], upper), pileup_ref.contigs_text(contigs, world["cname"], clen)


def test_the_two_files_equal_the_restatement(world):
    run = world["runs"]["loose"]
    want = _expected(world, run, 1, 0.0)
    assert run[".pileup"] == want[0] and run[".pileup.contigs"] == want[1]
    alts = {ln.split("\t")[3] for ln in run[".pileup"].decode().splitlines()}
    assert alts >= set("ACGT-+"), alts                            # the world is not degenerate
    for ln in run[".pileup"].decode().splitlines():                 # a site's count never exceeds its depth
        c = ln.split("\t")
        assert len(c) == 6 and 1 <= int(c[4]) <= int(c[5]), ln
    assert len(run[".pileup.contigs"].splitlines()) == 1 and int(run[".pileup.contigs"].split(b"\t")[2]) >= 50


def test_default_thresholds(world):
    run = world["runs"]["default"]
    want = _expected(world, world["runs"]["loose"], 3, 0.2)
    assert run[".pileup"] == want[0] and run[".pileup.contigs"] == want[1]
    lines = run[".pileup"].decode().splitlines()
    assert 20 <= len(lines) < len(world["runs"]["loose"][".pileup"].splitlines())
    assert all(int(ln.split("\t")[4]) >= 3 and 5 * int(ln.split("\t")[4]) >= int(ln.split("\t")[5]) for ln in lines)
    assert ".paf" not in run and ".editDistances" in run            # --pileup implies --edit-distance, nothing else


def test_every_other_file_is_the_file_of_the_run_without_the_flag(world):
    a, b = world["runs"]["paf"], world["runs"]["loose"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    a, b = world["runs"]["all_paf"], world["runs"]["all"]
    assert set(b) == set(a) | set(OURS)
    for suf in SAME + CLASSIFY_SUFFIXES + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    assert len(a[".EM.WIMP"]) > 100


@pytest.mark.parametrize("tag", ["all", "two", "merges", "bam"])
def test_the_same_files_in_every_variant(world, tag):
    a, b = world["runs"]["loose"], world["runs"][tag]
    for suf in OURS:
        assert b[suf] == a[suf], (tag, suf)
    if tag == "all":                                                # a read with several records counts once: the restatement on this run's own files
        want = _expected(world, b, 1, 0.0)
        assert b[".pileup"] == want[0] and b[".pileup.contigs"] == want[1]
    if tag == "bam":
        assert ".bam" in b and len(b[".bam"]) > 1000


def test_refused_combinations(world, tmp_path):
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["paf"][""])
    for args in (["mapDirectly", "--pileup", "--hpc", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup", "--shard-index", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup", "--stream-chunks", "--maxmemory-bytes", "100000", "-r", fasta, "-q", q, "-o", x],
                 ["index", "--pileup", "-r", fasta, "-i", x],
                 ["mapAgainstIndex", "--pileup", "-i", x, "-q", q, "-o", x],
                 ["classify", "--pileup", "--DB", db.dir, "--mappings", maps],
                 ["mapDirectly", "--pileup", "--pileup-min-count", "0", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup", "--pileup-min-frac", "1.5", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup-min-count", "2", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup-min-frac", "0.5", "-r", fasta, "-q", q, "-o", x]):
        p = _run(args)
        assert p.returncode == 1 and "--pileup" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
