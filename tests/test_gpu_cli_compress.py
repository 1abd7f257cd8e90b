"""`mapDirectly / mapAgainstIndex --compress-output` and `classify` from PREFIX.gz, on the small synthetic database of metamaps_amd/synth.py:
PREFIX.gz is BGZF that gunzips to the plain run's PREFIX byte for byte on every placement, the side files are identical, no plain PREFIX is
left, the file ends in BGZF's end-of-file block; classify from PREFIX.gz alone writes the seven .EM* files of classify from the plain file;
--then-classify --compress-output equals the two-step run; a damaged PREFIX.gz ends the run with the compressed offset in the message."""
import gzip
import os
import random
import shutil
import subprocess

import pytest

import deflate_corpus as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metamaps_amd", "csrc", "metamaps")
SIDE = (".meta", ".meta.unmappedReadsLengths")
EM = (".EM", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.WIMP", ".EM.lengthAndIdentitiesPerMappingUnit", ".EM.contigCoverage", ".EM.evidenceUnknownSpecies")


def _run(args, env=None, ok=True):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
    if ok:
        assert p.returncode == 0, p.stderr[-3000:]
    return p


def _params(prefix):
    return [l for l in open(prefix + ".parameters") if not l.startswith("outFileName")]


def _check_pair(plain, comp):
    """comp.gz against the plain run's files"""
    assert not os.path.exists(comp)
    raw = open(comp + ".gz", "rb").read()
    assert raw.endswith(dc.EOF_BLOCK)
    text = open(plain, "rb").read()
    assert gzip.decompress(raw) == text and len(text) > 1000
    dc.members(raw)
    for suf in SIDE:
        assert open(plain + suf, "rb").read() == open(comp + suf, "rb").read(), suf
    assert _params(plain) == _params(comp)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("cz")
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7)
    r1 = synth.make_reads(db, str(d / "r1.fq"), n_reads=400, read_len=3000, seed=3)
    r2 = synth.make_reads(db, str(d / "r2.fq"), n_reads=90, read_len=2500, seed=4)
    plain = str(d / "plain")
    _run(["mapDirectly", "--all", "-r", db.fasta, "-q", r1["path"], "-o", plain])
    _run(["classify", "--DB", db.dir, "--mappings", plain, "--minreads", "3"])
    return d, db, r1["path"], r2["path"], plain


@pytest.mark.parametrize("extra,env", [
    ([], {}),
    ([], {"MM_CLI_BATCH_READS": "37"}),                          # many batches: many short last blocks, concatenated in order
    ([], {"MM_DEFLATE_HOST": "1"}),
    (["--devices", "0,0"], {"MM_CLI_BATCH_READS": "50"}),
    (["--maxmemory-bytes", "1000000", "--shard-index"], {}),
    (["--maxmemory-bytes", "1000000", "--shard-index", "--devices", "0,0"], {"MM_CLI_BATCH_READS": "50"}),
    (["--maxmemory-bytes", "1000000", "--stream-chunks"], {}),
], ids=["replicated", "small_batches", "host_deflate", "two_contexts", "shard_index", "shard_index_two", "stream_chunks"])
def test_compressed_output_gunzips_to_the_plain_file(data, tmp_path, extra, env):
    d, db, r1, _, plain = data
    ref = plain
    if extra and extra[0] == "--maxmemory-bytes":                # (chunked references order a read's lines by chunk: compare like with like)
        ref = str(tmp_path / "ref")
        _run(["mapDirectly", "--all", "-r", db.fasta, "-q", r1, "-o", ref] + extra, env)
    comp = str(tmp_path / "comp")
    open(comp, "w").write("stale\n")                             # a plain PREFIX of an earlier run must not survive
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", r1, "-o", comp] + extra, env)
    _check_pair(ref, comp)


def test_two_query_files_and_map_against_index(data, tmp_path):
    d, db, r1, r2, plain = data
    q = r1 + "," + r2
    pl = [str(tmp_path / "pa"), str(tmp_path / "pb")]
    cz = [str(tmp_path / "ca"), str(tmp_path / "cb")]
    _run(["mapDirectly", "--all", "-r", db.fasta, "-q", q, "-o", ",".join(pl)])
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", q, "-o", ",".join(cz)])
    for a, b in zip(pl, cz):
        _check_pair(a, b)
    assert open(pl[0], "rb").read() == open(plain, "rb").read()
    _run(["index", "-r", db.fasta, "-i", str(tmp_path / "idx")])
    via = str(tmp_path / "via")
    _run(["mapAgainstIndex", "--all", "--compress-output", "-i", str(tmp_path / "idx"), "-q", r1, "-o", via])
    assert gzip.decompress(open(via + ".gz", "rb").read()) == open(plain, "rb").read() and not os.path.exists(via)


def _side_files_to(plain, prefix):
    for suf in SIDE + (".parameters",):
        shutil.copy(plain + suf, prefix + suf)


def _same_em(plain, prefix):
    for suf in EM:
        assert open(plain + suf, "rb").read() == open(prefix + suf, "rb").read(), suf
    assert os.path.getsize(plain + ".EM") > 100


@pytest.mark.parametrize("env", [{}, {"MM_CLASSIFY_THREADS": "7"}], ids=["default", "seven_pieces"])
def test_classify_from_gz_alone(data, tmp_path, env):
    d, db, r1, _, plain = data
    comp = str(tmp_path / "comp")
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", r1, "-o", comp])
    assert not os.path.exists(comp)
    _run(["classify", "--DB", db.dir, "--mappings", comp, "--minreads", "3"], env)
    _same_em(plain, comp)


@pytest.mark.parametrize("where", ["gz_beside", "bgzf_under_the_plain_name"])
def test_classify_from_a_file_bgzipped_elsewhere(data, tmp_path, where):
    """blocks of odd sizes written by Python's zlib (bam_writer.bgzf_block), not by this project"""
    import bam_writer as bw
    d, db, r1, _, plain = data
    text = open(plain, "rb").read()
    rng = random.Random(2)
    raw, at = b"", 0
    while at < len(text):
        n = rng.choice([1, 777, 12345, 65280, 65535, 30001])
        raw += bw.bgzf_block(text[at:at + n], level=rng.choice([1, 6, 9])); at += n
    raw += dc.EOF_BLOCK
    assert gzip.decompress(raw) == text
    pre = str(tmp_path / "other")
    open(pre + (".gz" if where == "gz_beside" else ""), "wb").write(raw)
    _side_files_to(plain, pre)
    _run(["classify", "--DB", db.dir, "--mappings", pre, "--minreads", "3"])
    _same_em(plain, pre)


def test_plain_file_is_preferred_and_plain_gzip_is_refused(data, tmp_path):
    d, db, r1, _, plain = data
    pre = str(tmp_path / "both")
    shutil.copy(plain, pre)
    open(pre + ".gz", "wb").write(b"not a gzip file at all")
    _side_files_to(plain, pre)
    _run(["classify", "--DB", db.dir, "--mappings", pre, "--minreads", "3"])
    _same_em(plain, pre)
    pg = str(tmp_path / "pg")
    open(pg + ".gz", "wb").write(gzip.compress(open(plain, "rb").read()))
    _side_files_to(plain, pg)
    p = _run(["classify", "--DB", db.dir, "--mappings", pg, "--minreads", "3"], ok=False)
    assert p.returncode != 0 and "plain gzip" in p.stderr and not os.path.exists(pg + ".EM")


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_then_classify_with_compressed_output_equals_two_steps(data, tmp_path, devices):
    d, db, r1, _, plain = data
    dev = ["--devices", devices, "--em-host-reduce"] if devices else []
    two, one, ff = str(tmp_path / "two"), str(tmp_path / "one"), str(tmp_path / "ff")
    _run(["mapDirectly", "--all", "-r", db.fasta, "-q", r1, "-o", two] + dev)
    _run(["classify", "--DB", db.dir, "--mappings", two, "--minreads", "3"] + dev)
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", r1, "-o", one, "--then-classify", db.dir, "--minreads", "3"] + dev)
    _check_pair(two, one)
    _same_em(two, one)
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", r1, "-o", ff, "--then-classify", db.dir, "--minreads", "3"] + dev,
         {"MM_CLI_CLASSIFY_FROM_FILE": "1"})                      # ... and when the in-process classify reads PREFIX.gz back
    _same_em(two, ff)


def test_damaged_files_name_the_offset(data, tmp_path):
    d, db, r1, _, plain = data
    comp = str(tmp_path / "comp")
    _run(["mapDirectly", "--all", "--compress-output", "-r", db.fasta, "-q", r1, "-o", comp], {"MM_CLI_BATCH_READS": "60"})
    raw = open(comp + ".gz", "rb").read()
    ms = dc.members(raw)
    assert len(ms) >= 4
    starts = [sum(len(m) for m in ms[:i]) for i in range(len(ms))]
    k = len(ms) // 2
    flip_at = starts[k] + len(ms[k]) // 2                        # inside the deflate data of block k
    flipped = bytearray(raw); flipped[flip_at] ^= 0x20
    bad = str(tmp_path / "flipped")
    open(bad + ".gz", "wb").write(bytes(flipped)); _side_files_to(comp, bad)
    p = _run(["classify", "--DB", db.dir, "--mappings", bad, "--minreads", "3"], ok=False)
    assert p.returncode != 0 and f"at byte {starts[k]}" in p.stderr, p.stderr[-2000:]
    cut = str(tmp_path / "cut")
    open(cut + ".gz", "wb").write(raw[:starts[k] + len(ms[k]) // 3]); _side_files_to(comp, cut)
    p = _run(["classify", "--DB", db.dir, "--mappings", cut, "--minreads", "3"], ok=False)
    assert p.returncode != 0 and f"truncated BGZF block at byte {starts[k]}" in p.stderr, p.stderr[-2000:]
    assert not os.path.exists(bad + ".EM") and not os.path.exists(cut + ".EM")


def test_flag_is_refused_where_it_does_not_belong(data, tmp_path):
    d, db, r1, _, plain = data
    p = _run(["classify", "--compress-output", "--DB", db.dir, "--mappings", plain], ok=False)
    assert p.returncode != 0 and "--compress-output" in p.stderr
