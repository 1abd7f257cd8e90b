"""`mapDirectly --extract-unmapped --extract-mapped --extract-taxa LIST --deplete-taxa LIST`: the four read files beside outputs that are byte for byte those
of the same run without the flags.  The world: four genomes of 30 kb, two of them the reference; 120 reads of 2 kb from all four (an N run and a lower-case read
among them), 20 reads of random bases, 10 reads shorter than k, as FASTQ with seeded qualities and header comments, and the same reads as unaligned BAM with
every other record stored reverse-complemented.  Every file inflates to what tests/reads_out_ref.py gives from that run's own PREFIX and the read list."""
import gzip
import os
import random

import numpy as np
import pytest

import bam_writer
import reads_out_ref as ref
from test_gpu_cli import CLI
from test_gpu_cli_edit_distance import _run, _take
from test_gpu_cli_qual import qual_record_bytes

pytestmark = pytest.mark.gpu
LABELS = ("unmapped", "mapped", "taxa", "depleted")
SUF_FQ = {k: f".{k}.fq.gz" for k in LABELS}
SUF_FA = {k: f".{k}.fa.gz" for k in LABELS}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from metamaps_amd import synth
    assert os.path.exists(CLI)
    d = tmp_path_factory.mktemp("extractcli")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11)
    in_ref = [c for g in (0, 1) for c in db.genome_contigs[g]]
    fasta = str(d / "ref.fa")
    with open(fasta, "wb") as f:
        for c in in_ref:
            f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    taxa = [db.genome_taxon[1]]
    assert taxa[0].startswith("x")                                   # (an x-prefixed ID, as buildDB.pl mints them)
    rd = synth.make_reads(db, str(d / "sampled.fq"), n_reads=120, read_len=2000, seed=5, frac_random=0.0, frac_short=0.0, abundance_sigma=0.3)
    lines = open(rd["path"], "rb").read().split(b"\n")
    recs = [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]          # (header with its comment, bases)
    rng = random.Random(17)
    recs += [(f"random{i}/none extra=1".encode(), "".join(rng.choice("ACGT") for _ in range(2000)).encode()) for i in range(20)]
    recs += [(f"short{i}".encode(), "".join(rng.choice("ACGT") for _ in range(5 + i)).encode()) for i in range(10)]
    rng.shuffle(recs)
    assert any(b != b.upper() for _, b in recs) and any(b"N" in b.upper() for _, b in recs)
    qrng = np.random.default_rng(23)
    ids = [h.split()[0].decode() for h, _ in recs]
    reads = [b for _, b in recs]
    quals = [list(qrng.integers(0, 94, size=len(b)).astype(np.uint8)) for b in reads]
    fq = str(d / "r.fq")
    with open(fq, "wb") as f:
        for (h, b), q in zip(recs, quals):
            f.write(b"@" + h + b"\n" + b + b"\n+\n" + bytes(v + 33 for v in q) + b"\n")
    ubam = str(d / "r.bam")
    bam_writer.write_bgzf(ubam, bam_writer.header_bytes() + b"".join(
        qual_record_bytes(n, b.decode().upper(), bytes(q), 0x10 if k % 2 else 0) for k, (n, b, q) in enumerate(zip(ids, reads, quals))), 20000)
    prefix = str(d / "out")
    flags = ["--extract-unmapped", "--extract-mapped", "--extract-taxa", ",".join(taxa), "--deplete-taxa", ",".join(taxa)]
    bq = ["--base-qualities"]
    base = ["mapDirectly", "-r", fasta, "-o", prefix]
    runs = {}
    for tag, q, extra, env in (("plain", fq, [], None), ("fq", fq, flags + bq, None), ("fa", fq, flags, None),
                               ("two", fq, flags + bq + ["--devices", "0,0"], {"MM_CLI_BATCH_READS": "7"}), ("two_plain", fq, ["--devices", "0,0"], {"MM_CLI_BATCH_READS": "7"}),
                               ("bam", ubam, flags + bq, None), ("bam_plain", ubam, [], None),
                               ("all", fq, ["--all"] + flags + bq, None), ("all_plain", fq, ["--all"], None),
                               ("side", fq, ["--bam", "--pileup"] + flags + bq, None), ("side_plain", fq, ["--bam", "--pileup"] + bq, None),
                               ("gz", fq, ["--compress-output"] + flags + bq, None), ("gz_plain", fq, ["--compress-output"], None),
                               ("long", fq, ["-m", "5000"] + flags + bq, None), ("long_plain", fq, ["-m", "5000"], None),
                               ("floor", fq, ["--pileup", "--min-base-quality", "10"] + flags, None), ("floor_plain", fq, ["--pileup", "--min-base-quality", "10"], None)):
        p = _run(base + ["-q", q] + extra, env)
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:], p.stdout.decode()[-2000:])
        runs[tag] = _take(prefix)
    return dict(d=d, fasta=fasta, fq=fq, base=base, prefix=prefix, flags=flags, taxa=taxa, ids=ids, reads=reads, quals=quals, runs=runs)


def _lines(run):
    text = gzip.decompress(run[".gz"]) if ".gz" in run else run[""]
    return text.decode().splitlines()


def _want(world, run, with_qual=True):
    sel = ref.selections(_lines(run), world["ids"], world["taxa"])
    names = [x.encode() for x in world["ids"]]
    return {k: ref.text(world["reads"], world["quals"], sel[k], [names[r] for r in sel[k]], with_qual) for k in LABELS}, sel


def _got(run, suffixes=SUF_FQ):
    out = {}
    for k in LABELS:
        data = run[suffixes[k]]
        assert data.endswith(ref.EOF_BLOCK)
        out[k] = gzip.decompress(data)
    return out


def test_the_world_is_not_degenerate(world):
    run = world["runs"]["fq"]
    meta = dict(ln.split() for ln in run[".meta"].decode().splitlines())
    assert int(meta["TotalReads"]) == len(world["ids"]) == 150
    assert int(meta["ReadsTooShort"]) >= 10 and int(meta["ReadsNotMapped"]) >= 10 and int(meta["ReadsMapped"]) >= 10
    prim = ref.primary_contigs(_lines(run))
    assert len({ref.taxon_of(c) for c in prim.values()}) >= 2
    _, sel = _want(world, run)
    assert len(sel["taxa"]) >= 5 and len(sel["mapped"]) - len(sel["taxa"]) >= 5


def test_every_file_is_the_restatement_of_its_own_run(world):
    for tag in ("fq", "two", "bam", "all", "side", "gz", "long"):
        run = world["runs"][tag]
        want, _ = _want(world, run)
        assert _got(run) == want, tag


def test_partitions_in_query_order(world):
    run = world["runs"]["fq"]
    _, sel = _want(world, run)
    n = len(world["ids"])
    assert sorted(sel["mapped"] + sel["unmapped"]) == list(range(n)) and sorted(sel["taxa"] + sel["depleted"]) == list(range(n))
    got = _got(run)
    ids = {k: [ln[1:] for ln in got[k].decode().split("\n")[0::4] if ln] for k in LABELS}
    for a, b in (("mapped", "unmapped"), ("taxa", "depleted")):
        assert sorted(ids[a] + ids[b], key=world["ids"].index) == world["ids"] and not set(ids[a]) & set(ids[b])
        for k in (a, b):
            assert ids[k] == sorted(ids[k], key=world["ids"].index)   # query order
    listed = [ln.split("\t")[1] for ln in run[".meta.unmappedReadsLengths"].decode().splitlines()]
    short = [x for x, b in zip(world["ids"], world["reads"]) if len(b) < 16]
    assert len(short) == 10 and set(listed) < set(ids["unmapped"]) and set(ids["unmapped"]) - set(listed) == set(short)


def test_the_same_bytes_from_small_batches_bam_all_and_other_side_outputs(world):
    first = _got(world["runs"]["fq"])
    for tag in ("two", "bam", "side", "gz"):
        assert _got(world["runs"][tag]) == first, tag
    got_all = _got(world["runs"]["all"])                             # under --all a read has more lines: the primary one decides `taxa`
    assert len(_lines(world["runs"]["all"])) > len(_lines(world["runs"]["fq"]))
    assert got_all == first


def test_fasta_without_base_qualities(world):
    run = world["runs"]["fa"]
    assert not any(s in run for s in SUF_FQ.values())
    want, _ = _want(world, run, with_qual=False)
    got = _got(run, SUF_FA)
    assert got == want and got["mapped"].startswith(b">") and b"\n+\n" not in got["mapped"]


def test_every_other_file_is_the_file_of_the_run_without_the_flags(world):
    for tag, plain, suffixes in (("fq", "plain", SUF_FQ), ("fa", "plain", SUF_FA), ("two", "two_plain", SUF_FQ), ("bam", "bam_plain", SUF_FQ), ("all", "all_plain", SUF_FQ),
                                 ("side", "side_plain", SUF_FQ), ("gz", "gz_plain", SUF_FQ), ("long", "long_plain", SUF_FQ)):
        a, b = world["runs"][plain], world["runs"][tag]
        assert set(b) == set(a) | set(suffixes.values()), tag
        for suf in a:
            assert a[suf] == b[suf], (tag, suf)
    assert ".bam" in world["runs"]["side"] and ".pileup" in world["runs"]["side"] and ".editDistances" not in world["runs"]["fq"]


def test_min_base_quality_implies_base_qualities_for_suffix_and_record(world):
    run = world["runs"]["floor"]
    assert not any(s in run for s in SUF_FA.values())
    assert _got(run) == _got(world["runs"]["fq"])                    # .fq.gz files that hold FASTQ records
    a = world["runs"]["floor_plain"]
    assert set(run) == set(a) | set(SUF_FQ.values())
    for suf in a:
        assert a[suf] == run[suf], suf


def test_min_length_above_every_read(world):
    run = world["runs"]["long"]
    assert _lines(run) == []
    got = _got(run)
    names = [x.encode() for x in world["ids"]]
    everything = ref.text(world["reads"], world["quals"], list(range(len(names))), names, True)
    assert got["unmapped"] == everything and got["depleted"] == everything
    assert run[SUF_FQ["mapped"]] == ref.EOF_BLOCK and run[SUF_FQ["taxa"]] == ref.EOF_BLOCK and len(ref.EOF_BLOCK) == 28


def test_the_mapped_file_maps_again_to_the_same_lines(world):
    first = world["runs"]["fq"]
    q = str(world["d"] / "again.mapped.fq.gz")
    open(q, "wb").write(first[SUF_FQ["mapped"]])
    p = _run(world["base"] + ["-q", q])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    again = _take(world["prefix"])
    assert again[""] == first[""] and len(first[""]) > 0


def test_refusals_name_their_flag(world):
    fasta, fq, prefix = world["fasta"], world["fq"], world["prefix"]
    one = {"--extract-unmapped": [], "--extract-mapped": [], "--extract-taxa": ["10000"], "--deplete-taxa": ["10000"]}
    for flag, val in one.items():
        for args in (["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, "--hpc"], ["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, "--shard-index"],
                     ["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, "--stream-chunks"], ["mapAgainstIndex", "-i", "nowhere", "-q", fq, "-o", prefix],
                     ["index", "-r", fasta, "-i", "nowhere"], ["classify", "--DB", "nowhere", "--mappings", prefix]):
            p = _run(args + [flag] + val)
            assert p.returncode != 0 and flag in (p.stderr + p.stdout).decode(), (flag, args)
    for flag in ("--extract-taxa", "--deplete-taxa"):
        for bad in ("", ",", "10000,", "10000,,x7001", "abc", "x", "12x", "x7001,x7001", "1 2", ",".join(str(i) for i in range(65))):
            p = _run(["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, flag, bad])
            assert p.returncode != 0 and flag in (p.stderr + p.stdout).decode(), (flag, bad)
    # a contig without a taxon ends the run before anything is mapped
    bare = str(world["d"] / "bare.fa")
    open(bare, "wb").write(b">contig_without_key\n" + b"ACGT" * 2000 + b"\n")
    p = _run(["mapDirectly", "-r", bare, "-q", fq, "-o", prefix, "--extract-taxa", "10000"])
    assert p.returncode != 0 and "Could not extract taxon ID" in (p.stderr + p.stdout).decode()
    p = _run(["mapDirectly", "-r", bare, "-q", fq, "-o", prefix, "--deplete-taxa", "10000", "--devices", "99"])   # said before any device is opened
    assert p.returncode != 0 and "Could not extract taxon ID" in (p.stderr + p.stdout).decode()
    p = _run(["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, "--base-qualities"])
    assert p.returncode != 0 and "--base-qualities needs" in (p.stderr + p.stdout).decode()
    assert _take(prefix) == {}
