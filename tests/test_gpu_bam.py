"""BAM queries on the GPU: a set uploaded as BAM's 4-bit codes (mm_seqset_add_nt16, packed on the device) is byte for byte the set uploaded
from the `samtools fastq` strings of the same records (mm_seqset_save files, mm_seqset_fetch_range), and the CLI writes the same files for
reads.bam as for the FASTQ `samtools fastq -n reads.bam` would give — mapDirectly (--all and best only), mapAgainstIndex, --then-classify,
two logical devices, and a comma list that mixes BAM and FASTQ.  BAM fixtures come from tests/bam_writer.py."""
import ctypes as C
import os
import random
import subprocess

import pytest

import bam_writer as bw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")
MM_ERR_STATE = -4


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _random_records(rng, n, long_reads=False):
    recs = []
    for i in range(n):
        L = rng.choice([0, 1, 15, 16, 17, 31, 32, 33, 200, 2500]) if i % 2 else rng.randrange(0, 4000)
        kind = i % 5
        if kind == 0:
            read = "".join(rng.choice(bw.NT16) for _ in range(L))
        elif kind == 1:                                           # long runs of one non-ACGT code, crossing words
            read = "".join(rng.choice("ACGT") for _ in range(L))
            if L > 40:
                a = rng.randrange(0, L - 20); b = min(L, a + rng.randrange(1, 3000))
                read = read[:a] + rng.choice("N=RY") * (b - a) + read[b:]
        else:
            read = "".join(rng.choice("ACGT" * 20 + "N") for _ in range(L))
        recs.append((bw.revcomp(read) if i % 3 == 0 else read, i % 3 == 0))   # (stored codes as letters, reverse)
    if long_reads:
        L = (4 << 20) + 1234                                       # crosses the host packer's 4-Mbase piece boundary
        recs.append(("".join(rng.choice("ACGT") for _ in range(L - 5000)) + "N" * 5000, False))
        recs.append(("ACGTRN" * (L // 6) + "NNN", True))
    return recs


def _as_sequenced(stored, rev):
    return bw.revcomp(stored) if rev else stored


@pytest.mark.parametrize("seed,long_reads", [(1, False), (2, False), (3, True)])
def test_nt16_upload_equals_ascii_upload(ctx, tmp_path, seed, long_reads):
    rng = random.Random(seed)
    recs = _random_records(rng, 300, long_reads)
    ascii_reads = [_as_sequenced(s, r).encode() for s, r in recs]
    A = ctx.seqset(ascii_reads)
    B = ctx.seqset_nt16([(bw.pack(s), len(s), r) for s, r in recs])
    pa, pb = str(tmp_path / "a.seqset"), str(tmp_path / "b.seqset")
    A.save(pa); B.save(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    buf, ln = B.fetch_range(0, B.count)
    assert list(ln) == [len(q) for q in ascii_reads]
    assert buf.tobytes() == b"".join(ascii_reads)
    A.close(); B.close()


@pytest.mark.parametrize("reads", [[], [b""], [b"", b"", b""], [b"ACGT" * 4], [b"N" * 16, b"N"], [b"=" * 17, b"", b"W" * 100]])
def test_nt16_upload_edge_sets(ctx, tmp_path, reads):
    A = ctx.seqset(reads)
    B = ctx.seqset_nt16([(bw.pack(q.decode()), len(q), False) for q in reads])
    pa, pb = str(tmp_path / "a.seqset"), str(tmp_path / "b.seqset")
    A.save(pa); B.save(pb)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    A.close(); B.close()


def test_mixing_ascii_and_nt16_is_a_state_error(ctx):
    from metamaps_amd import capi
    L = capi.lib()
    for first in ("ascii", "view", "nt16"):
        h = C.c_void_p()
        ctx.check(L.mm_seqset_create(ctx.h, C.byref(h)))
        codes = bw.pack("ACGTN")
        if first == "nt16":
            assert L.mm_seqset_add_nt16(h, codes, 5, 0) == 0
            assert L.mm_seqset_add(h, b"ACGT", 4) == MM_ERR_STATE
            assert L.mm_seqset_add_view(h, b"ACGT", 4) == MM_ERR_STATE
            assert L.mm_seqset_add_nt16(h, codes, 5, 1) == 0
        else:
            assert (L.mm_seqset_add(h, b"ACGT", 4) if first == "ascii" else L.mm_seqset_add_view(h, b"ACGT", 4)) == 0
            assert L.mm_seqset_add_nt16(h, codes, 5, 0) == MM_ERR_STATE
        assert L.mm_seqset_upload(h) == 0
        assert L.mm_seqset_add_nt16(h, codes, 5, 0) == MM_ERR_STATE   # frozen
        L.mm_seqset_destroy(h)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def _fastq_records(path):
    out = []
    with open(path) as f:
        while True:
            h = f.readline()
            if not h:
                break
            s = f.readline().strip(); f.readline(); f.readline()
            out.append((h[1:].split()[0], s.upper()))
    return out


def _bam_of(reads, path, rng, block_bytes=20000):
    """records of `reads` (name, read): some stored reverse-complemented (0x10), some with secondary/supplementary copies beside them,
    some with IUPAC codes; writes path.bam and the `samtools fastq -n` of it as path.fq; returns both paths"""
    recs = []
    for i, (n, s) in enumerate(reads):
        if i % 11 == 5 and len(s) > 300:
            s = s[:150] + "".join(rng.choice("RYKMSWBDHV=") for _ in range(30)) + s[180:]
        recs.append((n, s, 0x10 if i % 2 else 0))
        if i % 7 == 3:
            recs.append((n, s[: len(s) // 2], 0x100))
        if i % 9 == 4:
            recs.append((n, s[len(s) // 3:], 0x800 | 0x10))
    bw.write_bam(path + ".bam", recs, block_bytes=block_bytes)
    bw.write_fastq(path + ".fq", recs)
    return path + ".bam", path + ".fq"


SUFFIXES = ("", ".meta", ".meta.unmappedReadsLengths", ".parameters")
CLASSIFY_SUFFIXES = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")


def _same_files(a, b, subst, suffixes):
    for suf in suffixes:
        x = open(a + suf).read()
        y = open(b + suf).read()
        for u, v in subst:
            x = x.replace(u, v)
        assert x == y, (suf, a, b)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("bamcli")
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7)
    rng = random.Random(9)
    r1 = synth.make_reads(db, str(d / "r1_src.fq"), n_reads=220, read_len=3000, seed=3)
    r2 = synth.make_reads(db, str(d / "r2_src.fq"), n_reads=90, read_len=2500, seed=4)
    b1, f1 = _bam_of(_fastq_records(r1["path"]), str(d / "r1"), rng)
    b2, f2 = _bam_of(_fastq_records(r2["path"]), str(d / "r2"), rng, block_bytes=777)
    return {"db": db, "dir": d, "r1": (b1, f1), "r2": (b2, f2)}


def _map(args, env=None):
    p = subprocess.run([CLI] + args, capture_output=True, timeout=900, env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.mark.parametrize("mode", ["all", "best", "host_decode"])
def test_cli_map_directly_bam_equals_fastq(data, tmp_path, mode):
    db, (bam, fq) = data["db"], data["r1"]
    flags = [] if mode == "best" else ["--all"]
    env = {"MM_BAM_HOST_DECODE": "1"} if mode == "host_decode" else None
    _map(["mapDirectly"] + flags + ["-r", db.fasta, "-q", fq, "-o", str(tmp_path / "fq")])
    _map(["mapDirectly"] + flags + ["-r", db.fasta, "-q", bam, "-o", str(tmp_path / "bam")], env)
    assert os.path.getsize(str(tmp_path / "bam")) > 10000
    _same_files(str(tmp_path / "bam"), str(tmp_path / "fq"), [(bam, fq), (str(tmp_path / "bam"), str(tmp_path / "fq"))], SUFFIXES)


def test_cli_map_against_index_bam_equals_fastq(data, tmp_path):
    db, (bam, fq) = data["db"], data["r1"]
    _map(["index", "-r", db.fasta, "-i", str(tmp_path / "idx"), "--maxmemory-bytes", "1000000"])
    _map(["mapAgainstIndex", "--all", "-i", str(tmp_path / "idx"), "-q", fq, "-o", str(tmp_path / "fq")])
    _map(["mapAgainstIndex", "--all", "-i", str(tmp_path / "idx"), "-q", bam, "-o", str(tmp_path / "bam")])
    _same_files(str(tmp_path / "bam"), str(tmp_path / "fq"), [(bam, fq), (str(tmp_path / "bam"), str(tmp_path / "fq"))], SUFFIXES)


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_cli_then_classify_mixed_list_equals_fastq(data, tmp_path, devices):
    """a comma list of a BAM and a FASTQ, mapped and classified in one process, writes the files of the all-FASTQ list"""
    db = data["db"]
    (b1, f1), (b2, f2) = data["r1"], data["r2"]
    dev = ["--devices", devices, "--em-host-reduce"] if devices else []
    outs_fq = [str(tmp_path / "fq_a"), str(tmp_path / "fq_b")]
    outs_mix = [str(tmp_path / "mix_a"), str(tmp_path / "mix_b")]
    common = ["--then-classify", db.dir, "--minreads", "3"] + dev
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", f1 + "," + f2, "-o", ",".join(outs_fq)] + common)
    _map(["mapDirectly", "--all", "-r", db.fasta, "-q", b1 + "," + f2, "-o", ",".join(outs_mix)] + common, {"MM_CLI_BATCH_READS": "64"})
    subst = [(b1, f1)] + list(zip(outs_mix, outs_fq))
    for a, b in zip(outs_mix, outs_fq):
        _same_files(a, b, subst, SUFFIXES + CLASSIFY_SUFFIXES)
    assert os.path.getsize(outs_mix[0] + ".EM.WIMP") > 200


def test_cli_bam_errors(data, tmp_path):
    db, (bam, _) = data["db"], data["r1"]
    raw = open(bam, "rb").read()
    bad = str(tmp_path / "trunc.bam")
    open(bad, "wb").write(raw[: len(raw) // 2])
    p = subprocess.run([CLI, "mapDirectly", "-r", db.fasta, "-q", bad, "-o", str(tmp_path / "x")], capture_output=True, timeout=900)
    assert p.returncode != 0 and b"truncated BGZF block" in p.stderr, p.stderr[-1000:]
