"""`mapDirectly --vcf`: PREFIX.vcf beside outputs that stay byte for byte.  The reference is one contig of 30 kb that carries a homopolymer of 12, a
dinucleotide repeat of 10 units and a homopolymer of 300; the reads come from a strain copy with planted substitutions, deletions of 1, 3 and 30 bases,
insertions of 1, 5 and 30 bases and one deletion inside each repeat, with light noise.  PREFIX.vcf equals what tests/vcf_ref.py computes from the same run's
PREFIX (field 14 gives a read's primary record), .editDistances, .paf (the cg runs: other tests hold them to the naive walk), the reads and the reference,
at the thresholds 1 / 0 and at the defaults; the same bytes come out under --all --then-classify, from two logical devices in small batches, with the
accumulator merged every 50 triples, and together with --pileup --bam; the refused combinations name --vcf.  The planted truth itself, through perfect
alignments built from the planting, is held to the non-degeneracy conditions in a CPU test."""
import glob

import numpy as np
import pytest

import vcf_ref

LOOSE = ["--vcf-min-count", "1", "--vcf-min-frac", "0"]
SEED = 23
HP12, DI10, HP300, DEL30, INS30 = 5000, 10000, 15000, 4200, 8100                             # where the repeats start (the base before each is no part of it)
N_READS, READ_LEN = 200, 2000
I, D, EQ, X = 1, 2, 7, 8


def planted(seed=SEED):
    """the reference, the strain, and the strain as segments (op, n, ref pos, strain pos, bases) of its perfect alignment to the reference"""
    from metamaps_amd import synth
    rng = np.random.default_rng(seed)
    ref = bytearray(synth.random_genome(rng, 30_000).tobytes())
    ref[HP12 - 1:HP12 + 13] = b"C" + b"A" * 12 + b"G"
    ref[DI10 - 1:DI10 + 21] = b"T" + b"CA" * 10 + b"T"
    ref[HP300 - 1:HP300 + 301] = b"C" + b"A" * 300 + b"G"
    # The aligner minimises unit costs, and where a chance match ties it cuts a long indel into pieces (30 deleted random bases came out as 5D1=2D4=2D2=11D...).
    # So the two long indels are planted where nothing can tie: 30 deleted (inserted) bases of G and T between neighbours of A and C.
    pick = lambda letters, n: bytes(letters[int(x)] for x in rng.integers(0, 2, size=n))
    ref[DEL30 - 1:DEL30 + 62] = pick(b"AC", 1) + pick(b"GT", 30) + pick(b"AC", 32)
    ref[INS30 - 1:INS30 + 32] = pick(b"AC", 33)
    ref = bytes(ref)
    edits = {}                                                      # ref pos -> (kind, payload): a deletion removes ref[pos, pos + n), an insertion goes before ref[pos]
    for k in range(30):
        pos = 600 + 950 * k + int(rng.integers(0, 100))             # away from the repeats and the indels below
        edits[pos] = ("X", bytes([next(b for b in b"ACGT" if b != ref[pos])]))
    edits[2200], edits[3200], edits[DEL30] = ("D", 1), ("D", 3), ("D", 30)
    for pos, n in ((6100, 1), (7100, 5)):
        edits[pos] = ("I", synth.random_genome(rng, n).tobytes())
    edits[INS30] = ("I", pick(b"GT", 30))
    edits[HP12 + 11] = ("D", 1)                                     # the last A of the homopolymer: left-aligned to the C before it
    edits[DI10 + 18] = ("D", 2)                                     # the last CA unit
    edits[HP300 + 298] = ("D", 2)                                   # the last two A: 256 steps at most, and never past a read's first base
    assert len(edits) == 39
    segs, strain, r = [], bytearray(), 0

    def add(op, n, bases=b""):
        if segs and segs[-1][0] == op and op != I:
            segs[-1] = (op, segs[-1][1] + n, segs[-1][2], segs[-1][3], b"")
        else:
            segs.append((op, n, r, len(strain), bases))
    for pos in sorted(edits):
        kind, x = edits[pos]
        add(EQ, pos - r); strain += ref[r:pos]; r = pos
        if kind == "X":
            add(X, 1, x); strain += x; r += 1
        elif kind == "D":
            add(D, x); r += x
        else:
            add(I, len(x), x); strain += x
    add(EQ, len(ref) - r); strain += ref[r:]
    return ref, bytes(strain), segs, edits


def read_spans(seed=SEED):
    rng = np.random.default_rng(seed + 1)
    return [(int(s), int(rng.choice([-1, 1]))) for s in rng.integers(0, 30_000 - READ_LEN - 100, size=N_READS)]


def truth_jobs(ref, strain, segs, spans):
    """the perfect alignment of every noiseless read strain[s, s + READ_LEN) as a job of vcf_ref"""
    from metamaps_amd import synth
    jobs = []
    for s0, strand in spans:
        s1, runs, first = s0 + READ_LEN, [], None
        for op, n, r, s, _ in segs:
            if op == D:
                if s0 < s < s1:
                    runs.append((n, D))
                continue
            lo, hi = max(s, s0), min(s + n, s1)
            if lo >= hi:
                continue
            if first is None:
                first = r + (lo - s if op != I else 0)
            runs.append((hi - lo, op))
        read = strain[s0:s1]
        if strand < 0:
            read = synth.revcomp(np.frombuffer(read, dtype=np.uint8)).tobytes()
        jobs.append(dict(read=read, strand=strand, c=0, first=first, runs=[n << 4 | op for n, op in runs], d=0, use=1))
    return jobs


def non_degenerate(text, ref, edits, intervals):
    """the conditions on a default-threshold PREFIX.vcf; returns its lines"""
    lines = [ln.split("\t") for ln in text.decode().splitlines() if not ln.startswith("#")]
    assert all(len(c) == 8 and c[2] == c[5] == c[6] == "." for c in lines)
    info = [dict(kv.split("=") for kv in c[7].split(";")) for c in lines]
    assert all(1 <= int(i["AO"]) <= int(i["DP"]) for i in info)
    assert any(len(c[3]) == 1 and len(c[4]) == 1 for c in lines), "an SNV"
    assert any(len(c[3]) > 1 and len(c[4]) == 1 for c in lines), "an explicit DEL"
    assert any(len(c[3]) == 1 and len(c[4]) > 1 and c[4][0] != "<" for c in lines), "an explicit INS"
    assert any(c[1] == str(DEL30) and c[4] == "<DEL>" and i["SVTYPE"] == "DEL" and i["SVLEN"] == "-30" and i["END"] == str(DEL30 + 30) for c, i in zip(lines, info))
    assert any(c[1] == str(INS30) and c[4] == "<INS>" and i["SVTYPE"] == "INS" and i["SVLEN"] == "30" and i["END"] == str(INS30) for c, i in zip(lines, info))
    # the deleted last A of the homopolymer of 12 appears at the C before the homopolymer, eleven bases left of where it was planted
    assert ["1" for c in lines if c[1] == str(HP12) and c[3] == "CA" and c[4] == "C"] == ["1"] and edits[HP12 + 11] == ("D", 1)
    assert any(c[1] == str(DI10) and c[3] == "TCA" and c[4] == "T" for c in lines)
    snv = {int(c[1]) - 1: c[4] for c in lines if len(c[3]) == 1 and len(c[4]) == 1}
    deep = [pos for pos, (kind, _) in edits.items() if kind == "X" and vcf_ref.depth(intervals, 0, pos) >= 10]
    assert len(deep) >= 10 and all(snv.get(pos) == edits[pos][1].decode() for pos in deep)
    return lines


def test_the_planted_truth_is_not_degenerate():
    ref, strain, segs, edits = planted()
    assert len(strain) == len(ref) - 39 + 36 and ref[HP12 - 1:HP12 + 13] == b"C" + b"A" * 12 + b"G"
    jobs = truth_jobs(ref, strain, segs, read_spans())
    iv = [vcf_ref.interval(j) for j in jobs]
    t = vcf_ref.table(jobs, [ref])
    text = vcf_ref.vcf_text(vcf_ref.finish(t, iv, [ref], 3, 0.2), ["c"], [len(ref)])
    lines = non_degenerate(text, ref, edits, iv)
    assert len(lines) >= 35
    # the deletion at the end of the homopolymer of 300 is spread over several anchors: 256 steps at most, and never past a read's first base
    hp = sorted(int(c[1]) for c in lines if HP300 <= int(c[1]) <= HP300 + 300 and c[3] == "AAA" and c[4] == "A")
    assert len(hp) >= 1 and HP300 + 298 - 256 in hp


def build_world(d):
    """the reference, the reads and every run of the command line, in the directory d"""
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
    pl = ["--pileup", "--pileup-min-count", "1", "--pileup-min-frac", "0"]
    runs = {}
    for tag, extra, env in (("paf", ["--paf"], None), ("loose", ["--paf", "--vcf"] + LOOSE, None), ("default", ["--vcf"], None),
                            ("all_paf", classify + ["--paf"], None), ("all", classify + ["--paf", "--vcf"] + LOOSE, None),
                            ("two", ["--vcf", "--devices", "0,0"] + LOOSE, {"MM_CLI_BATCH_READS": "5"}),
                            ("merges", ["--vcf"] + LOOSE, {"MM_VCF_MERGE_PAIRS": "50"}),
                            ("pileup_bam", ["--bam"] + pl, None), ("combo", ["--bam", "--vcf", "--compress-output"] + pl + LOOSE, None),
                            ("empty", ["--vcf", "-m", "5000"], None)):
        p = _run(base + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(db=db, reads=reads, cname=cname, contigs=[ref], edits=edits, runs=runs, fasta=fasta, q=q)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return build_world(tmp_path_factory.mktemp("vcfcli"))


def _expected(world, run, min_count, min_frac):
    from test_gpu_cli_pileup import _jobs
    jobs = [j for j in _jobs(world, run) if j["use"]]
    iv = [vcf_ref.interval(j) for j in jobs]
    t = vcf_ref.table(jobs, world["contigs"])
    return vcf_ref.vcf_text(vcf_ref.finish(t, iv, world["contigs"], min_count, min_frac), world["cname"], [len(c) for c in world["contigs"]]), iv


@pytest.mark.gpu
def test_the_file_equals_the_restatement(world):
    run = world["runs"]["loose"]
    want, iv = _expected(world, run, 1, 0.0)
    assert run[".vcf"] == want and len(iv) >= 150
    assert run[".vcf"].startswith(vcf_ref.header_text(world["cname"], [30_000])) and len(run[".vcf"].splitlines()) > 200


@pytest.mark.gpu
def test_default_thresholds_and_non_degeneracy(world):
    run = world["runs"]["default"]
    want, iv = _expected(world, world["runs"]["loose"], 3, 0.2)
    assert run[".vcf"] == want
    lines = non_degenerate(run[".vcf"], world["contigs"][0], world["edits"], iv)
    assert 35 <= len(lines) < len(world["runs"]["loose"][".vcf"].splitlines()) - 13
    assert all(int(c[7].split(";")[1][3:]) >= 3 and 5 * int(c[7].split(";")[1][3:]) >= int(c[7].split(";")[0][3:]) for c in lines)
    assert ".paf" not in run and ".pileup" not in run and ".editDistances" in run   # --vcf implies --edit-distance, nothing else


@pytest.mark.gpu
def test_every_other_file_is_the_file_of_the_run_without_the_flag(world):
    from test_gpu_cli import CLASSIFY_SUFFIXES
    from test_gpu_cli_edit_distance import SAME
    a, b = world["runs"]["paf"], world["runs"]["loose"]
    assert set(b) == set(a) | {".vcf"}
    for suf in SAME + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    a, b = world["runs"]["all_paf"], world["runs"]["all"]
    assert set(b) == set(a) | {".vcf"}
    for suf in SAME + CLASSIFY_SUFFIXES + (".editDistances", ".paf"):
        assert a[suf] == b[suf], suf
    assert len(a[".EM.WIMP"]) > 100
    a, b = world["runs"]["pileup_bam"], world["runs"]["combo"]
    assert ".gz" in b and set(b) - {".gz"} == (set(a) - {""}) | {".vcf"}
    for suf in (".pileup", ".pileup.contigs", ".bam", ".editDistances", ".meta"):
        assert a[suf] == b[suf], suf


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["all", "two", "merges", "combo"])
def test_the_same_bytes_in_every_variant(world, tag):
    a, b = world["runs"]["loose"], world["runs"][tag]
    assert b[".vcf"] == a[".vcf"], tag
    if tag == "all":                                                # a read with several records counts once: the restatement on this run's own files
        assert b[".vcf"] == _expected(world, b, 1, 0.0)[0]
    if tag == "combo":
        assert len(b[".bam"]) > 1000 and len(b[".pileup"]) > 1000 and not b[".vcf"].startswith(b"\x1f\x8b")   # plain text under --compress-output


@pytest.mark.gpu
def test_an_empty_run_writes_the_header_alone(world):
    run = world["runs"]["empty"]                                    # no read is as long as -m asks
    assert run[".vcf"] == vcf_ref.header_text(world["cname"], [30_000]) and run.get("", b"") == b""


@pytest.mark.gpu
def test_refused_combinations(world, tmp_path):
    from test_gpu_cli_edit_distance import _run
    db, q, fasta, x = world["db"], world["q"], world["fasta"], str(tmp_path / "x")
    maps = str(tmp_path / "m")
    open(maps, "wb").write(world["runs"]["paf"][""])
    for args in (["mapDirectly", "--vcf", "--hpc", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--vcf", "--shard-index", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--vcf", "--stream-chunks", "--maxmemory-bytes", "100000", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--vcf", "--pileup", "--hpc", "-r", fasta, "-q", q, "-o", x],
                 ["index", "--vcf", "-r", fasta, "-i", x],
                 ["mapAgainstIndex", "--vcf", "-i", x, "-q", q, "-o", x],
                 ["classify", "--vcf", "--DB", db["dir"], "--mappings", maps],
                 ["mapDirectly", "--vcf", "--vcf-min-count", "0", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--vcf", "--vcf-min-frac", "1.5", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--vcf-min-count", "2", "-r", fasta, "-q", q, "-o", x],
                 ["mapDirectly", "--pileup", "--vcf-min-frac", "0.5", "-r", fasta, "-q", q, "-o", x]):
        p = _run(args)
        assert p.returncode == 1 and "--vcf" in p.stderr.decode(), (args, p.stderr.decode()[-500:])
        assert glob.glob(x + "*") == [] and glob.glob(maps + ".*") == [], args
