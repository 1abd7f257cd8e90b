"""`mapDirectly --hpc` end to end.  By definition it is today's pipeline on homopolymer-compressed sequences with lengths and coordinates reported
raw: so a run with --hpc on raw files must equal a run without it on files compressed in Python, with fields 2, 4, 7, 8, 9 of every line
translated by the Python map; and that run must equal the oracle CLI on the compressed files."""
import gzip
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")
PARAMS = ["-k", "16", "-w", "8", "-m", "1000", "--pi", "80"]
CLASSIFY_SUFFIXES = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")


def hpc(s: bytes):
    """(compressed bytes, raw position of the first base of every run, of the last)"""
    out, first, last, at = bytearray(), [], [], 0
    for ch, grp in itertools.groupby(s.upper()):
        n = len(list(grp))
        out.append(ch); first.append(at); last.append(at + n - 1)
        at += n
    return bytes(out), first, last


def dup30(rng, s: np.ndarray) -> np.ndarray:
    return np.repeat(s, 1 + (rng.random(len(s)) < 0.3))


def read_fastq(path):
    recs = []
    with open(path, "rb") as f:
        while True:
            h = f.readline()
            if not h:
                break
            recs.append((h[1:].split()[0], f.readline().strip()))
            f.readline(); f.readline()
    return recs


def write_fastq(path, recs):
    with open(path, "wb") as f:
        for name, s in recs:
            f.write(b"@" + name + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


class World:
    """the homopolymer-enriched DB, its reads, their compressed twins and the Python maps"""
    def __init__(self, d):
        from metamaps_amd import synth
        rng = np.random.default_rng(21)
        genomes = []
        for g in range(10):
            base = synth.random_genome(rng, 154_000) if g % 2 == 0 else synth.mutate(rng, genomes[-1][1], sub=0.03)
            genomes.append((g, base))
        contigs = []
        for g, base in genomes:                                     # 10 genomes x about 200 kb after 30 % of the positions are duplicated
            s = dup30(np.random.default_rng(100 + g), base).copy()
            if g == 2:
                s[5000:5600] = ord("N"); s[9000:9400] = np.frombuffer(s[9000:9400].tobytes().lower(), dtype=np.uint8); s[20000:20003] = ord("R")
            cut = len(s) // 3
            contigs += [(g, s[:cut].tobytes()), (g, s[cut:].tobytes())]
        self.db = synth.write_db_dir(os.path.join(d, "db"), contigs)
        self.contig_name = [f"C{ci}|kraken:taxid|{1000000 + g}|SYN{ci:05d}.1" for ci, (g, _) in enumerate(contigs)]
        self.contig = {n: hpc(s) + (len(s),) for n, (_, s) in zip(self.contig_name, contigs)}
        sdb = synth.SynthDB(self.db["dir"], self.db["fasta"], self.contig_name, [str(1000000 + g) for g, _ in contigs],
                            [np.frombuffer(s, dtype=np.uint8) for _, s in contigs], [str(1000000 + g) for g in range(10)], [[2 * g, 2 * g + 1] for g in range(10)])
        self.sdb = sdb
        self.reads = synth.make_reads(sdb, os.path.join(d, "reads.fq"), n_reads=300, read_len=5000, seed=3)["path"]
        self.recs = read_fastq(self.reads)
        self.rawlen = {n: len(s) for n, s in self.recs}
        self.db_c = os.path.join(d, "DBc.fa")
        with open(self.db_c, "wb") as f:
            for n, (_, s) in zip(self.contig_name, contigs):
                f.write(b">" + n.encode() + b"\n" + hpc(s)[0] + b"\n")
        self.reads_c = os.path.join(d, "reads_c.fq")
        write_fastq(self.reads_c, [(n, hpc(s)[0]) for n, s in self.recs])

    def translate(self, line: str) -> str:
        """a mapping line of the run on compressed files -> the line --hpc must write"""
        f = line.split(" ")
        comp, first, last, rawlen = self.contig[f[5]]
        cl, rl = len(comp), self.rawlen[f[0].encode()]
        s, e = int(f[7]), int(f[8])
        f[1], f[3], f[6] = str(rl), str(rl - 1), str(rawlen)
        f[7] = str(first[s] if s < cl else rawlen + s - cl)
        f[8] = str(last[e] if e < cl else rawlen + e - cl)
        return " ".join(f)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(str(tmp_path_factory.mktemp("hpcw")))


def run(args, env=None, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, timeout=900, env=dict(os.environ, **(env or {})))
    if ok:
        assert p.returncode == 0, p.stderr.decode()[-1500:]
    return p


def check_equivalent(world, pre_c, pre_h, recs=None):
    rawlen = {n: len(s) for n, s in (recs or world.recs)}
    lc, lh = open(pre_c).read().splitlines(), open(pre_h).read().splitlines()
    assert len(lc) == len(lh) and len(lc) > 0
    for i, (a, b) in enumerate(zip(lc, lh)):
        assert world.translate(a) == b, (i, a, b)
    assert open(pre_c + ".meta").read() == open(pre_h + ".meta").read()
    uc = [l.split("\t") for l in open(pre_c + ".meta.unmappedReadsLengths").read().splitlines()]
    uh = [l.split("\t") for l in open(pre_h + ".meta.unmappedReadsLengths").read().splitlines()]
    assert [u[1] for u in uc] == [u[1] for u in uh]
    assert [int(u[0]) for u in uh] == [rawlen[u[1].encode()] for u in uh]           # raw lengths


@pytest.fixture(scope="module")
def base_runs(world, tmp_path_factory):
    """the --all pair every other test compares with: without --hpc on the compressed files, with --hpc on the raw ones"""
    d = tmp_path_factory.mktemp("hpcr")
    pre_c, pre_h = str(d / "c"), str(d / "h")
    run(["mapDirectly", "--all", "-r", world.db_c, "-q", world.reads_c, "-o", pre_c] + PARAMS)
    run(["mapDirectly", "--all", "--hpc", "-r", world.db["fasta"], "-q", world.reads, "-o", pre_h] + PARAMS)
    return pre_c, pre_h


def test_equivalence_and_oracle(world, base_runs, oracle_lib, tmp_path):
    import orc
    pre_c, pre_h = base_runs
    check_equivalent(world, pre_c, pre_h)
    assert "hpc 1\n" in open(pre_h + ".parameters").read()
    assert any(int(a.split(" ")[1]) != int(world.translate(a).split(" ")[1]) for a in open(pre_c).read().splitlines()[:5])   # (the translation does change lines)
    pre_o = str(tmp_path / "o")
    subprocess.run([orc.CLI, "mapDirectly", "--all", "-r", world.db_c, "-q", world.reads_c, "-o", pre_o] + PARAMS, check=True, capture_output=True, timeout=900)
    lo, lc = open(pre_o).read().splitlines(), open(pre_c).read().splitlines()
    assert len(lo) >= 200 and len({l.split(" ")[0] for l in lo}) >= len(world.recs) // 2          # the oracle alone maps at least half of the reads
    assert len(lo) == len(lc)
    for i, (a, b) in enumerate(zip(lo, lc)):
        fa, fb = a.split(" "), b.split(" ")
        assert fa[:13] == fb[:13], (i, a, b)
        assert abs(float(fa[13]) - float(fb[13])) <= 2e-6 + 1e-5 * max(abs(float(fa[13])), abs(float(fb[13]))), (i, a, b)
    for suf in (".meta", ".meta.unmappedReadsLengths"):
        assert open(pre_o + suf).read() == open(pre_c + suf).read(), suf


MODES = {   # mode: (flags of both runs, flags of the --hpc run alone, its environment, whether the run on the compressed files is the module's --all pair)
    "best": ([], [], {}, False),
    "devices": (["--all"], ["--devices", "0,0"], {"MM_CLI_BATCH_READS": "64"}, True),
    "gzip": (["--all"], [], {}, True),
    "compress": (["--all"], ["--compress-output"], {}, True),
    "chunks": (["--all", "--maxmemory-bytes", "5000000"], [], {}, False),
    "shard": (["--all", "--maxmemory-bytes", "5000000"], ["--shard-index", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "100"}, False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_modes(world, base_runs, tmp_path, mode):
    both, only_h, env, reuse = MODES[mode]
    pre_c, pre_h, q_h = str(tmp_path / "c"), str(tmp_path / "h"), world.reads
    if mode == "gzip":
        q_h = str(tmp_path / "h.fq.gz")
        with open(world.reads, "rb") as f, gzip.open(q_h, "wb", compresslevel=1) as g:
            g.write(f.read())
    if reuse:
        pre_c = base_runs[0]
    else:
        p = run(["mapDirectly"] + both + ["-r", world.db_c, "-q", world.reads_c, "-o", pre_c] + PARAMS)
        assert ("index chunk 2/" in p.stdout.decode()) == ("--maxmemory-bytes" in both)   # several chunks on this small DB
    p = run(["mapDirectly", "--hpc"] + both + only_h + ["-r", world.db["fasta"], "-q", q_h, "-o", pre_h] + PARAMS, env=env)
    assert ("index chunk 2/" in p.stdout.decode()) == ("--maxmemory-bytes" in both)
    if mode == "compress":
        assert not os.path.exists(pre_h)
        with open(pre_h, "wb") as f:
            f.write(gzip.open(pre_h + ".gz", "rb").read())
    check_equivalent(world, pre_c, pre_h)


def test_two_query_files(world, tmp_path):
    half = len(world.recs) // 2
    parts = [world.recs[:half], world.recs[half:]]
    qc, qh, oc, oh = [], [], [], []
    for j, recs in enumerate(parts):
        qh.append(str(tmp_path / f"h{j}.fq")); write_fastq(qh[-1], recs)
        qc.append(str(tmp_path / f"c{j}.fq")); write_fastq(qc[-1], [(n, hpc(s)[0]) for n, s in recs])
        oc.append(str(tmp_path / f"oc{j}")); oh.append(str(tmp_path / f"oh{j}"))
    run(["mapDirectly", "--all", "-r", world.db_c, "-q", ",".join(qc), "-o", ",".join(oc)] + PARAMS)
    run(["mapDirectly", "--all", "--hpc", "-r", world.db["fasta"], "-q", ",".join(qh), "-o", ",".join(oh)] + PARAMS)
    for j in range(2):
        check_equivalent(world, oc[j], oh[j], parts[j])


def test_then_classify_equals_separate_classify(world, base_runs, tmp_path):
    _, pre_h = base_runs
    run(["classify", "--DB", world.db["dir"], "--mappings", pre_h, "--minreads", "3"])
    one = str(tmp_path / "one")
    run(["mapDirectly", "--all", "--hpc", "-r", world.db["fasta"], "-q", world.reads, "-o", one, "--then-classify", world.db["dir"], "--minreads", "3"] + PARAMS)
    for suf in ("", ".meta", ".meta.unmappedReadsLengths") + CLASSIFY_SUFFIXES:
        assert open(one + suf, "rb").read() == open(pre_h + suf, "rb").read(), suf
    assert os.path.getsize(one + ".EM.WIMP") > 200


def test_what_the_feature_is_for(world, tmp_path):
    """100 reads cut from the DB whose only edits are +-1 changes in the length of runs of length >= 2 (each with probability 0.5): with --hpc every read's
    best line is its source contig, with every sketch hash shared and identity 100"""
    rng = np.random.default_rng(5)
    names = [n for n in world.contig_name if world.contig[n][3] > 20000]
    seqs = dict(zip(world.contig_name, world.sdb.contig_seqs))
    recs, src = [], {}
    for r in range(100):
        cn = names[int(rng.integers(len(names)))]
        s = seqs[cn]
        a = int(rng.integers(6000, len(s) - 6000))
        while s[a] == s[a - 1] or b"N" in s[a:a + 5000].tobytes().upper():          # start on a run boundary, away from the N block
            a += 1
        piece = s[a:a + 5000].tobytes().upper()
        out = bytearray()
        for ch, grp in itertools.groupby(piece):
            n = len(list(grp))
            if n >= 2 and rng.random() < 0.5:
                n += 1 if rng.random() < 0.5 else -1
            out += bytes([ch]) * n
        name = f"hp{r:03d}".encode()
        recs.append((name, bytes(out))); src[name.decode()] = cn
    q = str(tmp_path / "hp.fq")
    write_fastq(q, recs)
    pre_h, pre_r = str(tmp_path / "h"), str(tmp_path / "r")
    run(["mapDirectly", "--hpc", "-r", world.db["fasta"], "-q", q, "-o", pre_h] + PARAMS)
    run(["mapDirectly", "-r", world.db["fasta"], "-q", q, "-o", pre_r] + PARAMS)
    best = {}
    for l in open(pre_h).read().splitlines():
        f = l.split(" ")
        if f[0] not in best or float(f[9]) > float(best[f[0]][9]):
            best[f[0]] = f
    assert len(best) == 100
    for name, f in best.items():
        assert f[5] == src[name] and f[10] == f[11] and f[9] == "100", f
    ids = [float(l.split(" ")[9]) for l in open(pre_r).read().splitlines()]
    print(f"without --hpc: {len(ids)} lines, mean identity {np.mean(ids) if ids else float('nan'):.2f}; with --hpc: 100 reads at identity 100")


def test_refusals_and_no_effect_without_the_flag(world, base_runs, tmp_path):
    for args in (["index", "--hpc", "-r", world.db_c, "-i", str(tmp_path / "idx")],
                 ["index", "--full-index", "--hpc", "-r", world.db_c, "-i", str(tmp_path / "idx")],
                 ["mapAgainstIndex", "--hpc", "-i", str(tmp_path / "idx"), "-q", world.reads, "-o", str(tmp_path / "x")],
                 ["classify", "--hpc", "--DB", world.db["dir"], "--mappings", base_runs[1]]):
        p = run(args, ok=False)
        assert p.returncode == 1 and "--hpc" in p.stderr.decode(), args
    assert not os.path.exists(str(tmp_path / "idx.index"))
    assert not any(l.split(" ")[0] == "hpc" for l in open(base_runs[0] + ".parameters").read().splitlines())   # no hpc line (paths may hold the letters)
