"""The outputs of `mapDirectly` side by side and one at a time: the two decisions every batch makes from the combination asked for — whether its alignments are
traced back or only measured, and when its reads leave the device (OutputPlan::traceback, ::reads_until_text; BatchSideOutputs::from_mapping, ::from_text).
Four genomes of 30 kb in two contigs each, every other one the reference (so some reads stay unmapped), 60 FASTQ reads of 2 kb with qualities, batches of 7
reads on two logical devices.  Six runs:
  all       every output at once
  edit      --edit-distance alone: no traceback, the reads released in from_mapping
  depth     --depth alone: no traceback, the reads kept to from_text
  sorted    --bam-sorted alone: traceback, from_text returns before the unsorted records
  extract   --extract-unmapped --extract-mapped alone: no alignment at all
  none      no flag
Every file of the last five is the file of the same name of the first (BGZF inflated), and PREFIX, .meta and .meta.unmappedReadsLengths are those of all six.
Two files cannot be the same bytes, because `all` carries --base-qualities and these runs cannot (alone it is refused beside --bam-sorted, and it changes the
read files' format): PREFIX.sorted.bam of `sorted` holds the same records with QUAL 0xFF, and its index is what tests/bai_ref.py builds from it; the read
files of `extract` are FASTA, the records of `all`'s FASTQ without their quality lines."""
import numpy as np
import pytest

import bai_ref
import bam_ref
import reads_out_ref
from test_gpu_cli_edit_distance import SAME, _run, _take

pytestmark = pytest.mark.gpu
READ_SEED = 9
BGZF = (".bam", ".sorted.bam", ".unmapped.fq.gz", ".mapped.fq.gz", ".unmapped.fa.gz", ".mapped.fa.gz")
ALL = ["--paf", "--bam", "--bam-sorted", "--pileup", "--vcf", "--consensus", "--depth", "--error-profile", "--base-qualities", "--extract-unmapped", "--extract-mapped"]
RUNS = (("all", ALL), ("edit", ["--edit-distance"]), ("depth", ["--depth"]), ("sorted", ["--bam-sorted"]), ("extract", ["--extract-unmapped", "--extract-mapped"]), ("none", []))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("together")
    db = synth.make_db(str(d / "db"), n_genomes=4, genome_len=30_000, seed=11, contigs_per_genome=2, with_oddities=False)
    rd = synth.make_reads(db, str(d / "r0.fq"), n_reads=60, read_len=2000, seed=READ_SEED)
    lines = open(rd["path"], "rb").read().split(b"\n")
    rng = np.random.default_rng(31)
    fq = str(d / "r.fq")
    with open(fq, "wb") as f:
        for i in range(0, len(lines) - 1, 4):
            f.write(lines[i].split()[0] + b"\n" + lines[i + 1] + b"\n+\n" + bytes(rng.integers(33, 127, size=len(lines[i + 1])).astype(np.uint8)) + b"\n")
    fasta = str(d / "even.fa")
    with open(fasta, "wb") as f:
        for g in range(0, len(db.genome_contigs), 2):
            for c in db.genome_contigs[g]:
                f.write(b">" + db.contig_ids[c].encode() + b"\n" + db.contig_seqs[c].tobytes() + b"\n")
    prefix, out = str(d / "out"), {"as written": {}}
    for tag, flags in RUNS:
        p = _run(["mapDirectly", "-r", fasta, "-q", fq, "-o", prefix, "--devices", "0,0"] + flags, {"MM_CLI_BATCH_READS": "7"})
        assert p.returncode == 0, (tag, p.stderr.decode()[-2000:])
        out["as written"][tag] = _take(prefix)
        out[tag] = {suf: reads_out_ref.inflate(data) if suf in BGZF else data for suf, data in out["as written"][tag].items()}
    return out


def test_the_world_is_not_degenerate(runs):
    a = runs["all"]
    meta = dict(ln.split() for ln in a[".meta"].decode().splitlines())
    assert int(meta["TotalReads"]) == 60 and int(meta["ReadsNotMapped"]) >= 1 and int(meta["ReadsMapped"]) >= 20
    assert len(a[".meta.unmappedReadsLengths"].splitlines()) == int(meta["ReadsNotMapped"])
    edit = [ln.split(" ") for ln in a[".editDistances"].decode().splitlines()]
    assert len(edit) == len(a[""].splitlines()) and any(e[3:] == ["NA", "NA", "NA"] for e in edit)
    assert len({e[1] for e in edit if e[3] != "NA"}) >= 2
    assert sorted(a) == sorted(SAME + (".editDistances", ".paf", ".bam", ".sorted.bam", ".sorted.bam.bai", ".pileup", ".pileup.contigs", ".vcf", ".consensus.fa", ".consensus.tsv",
                                       ".depth.bedgraph", ".depth.windows", ".depth.contigs", ".errorProfile.substitutions", ".errorProfile.indels", ".errorProfile.qualities",
                                       ".errorProfile.contigs", ".unmapped.fq.gz", ".mapped.fq.gz"))
    assert len(a[".paf"].splitlines()) >= 20 and len(a[".depth.bedgraph"].splitlines()) >= 20 and len(a[".errorProfile.qualities"].splitlines()) > 50


@pytest.mark.parametrize("tag, own", [("edit", [".editDistances"]), ("depth", [".editDistances", ".depth.bedgraph", ".depth.windows", ".depth.contigs"]), ("none", [])])
def test_every_file_is_the_file_of_the_run_with_every_output(runs, tag, own):
    a, b = runs["all"], runs[tag]
    assert sorted(b) == sorted(list(SAME) + own)
    for suf in b:
        assert b[suf] == a[suf], (tag, suf)


def test_the_sorted_bam_alone(runs):
    a, b = runs["all"], runs["sorted"]
    assert sorted(b) == sorted(list(SAME) + [".editDistances", ".sorted.bam", ".sorted.bam.bai"])
    for suf in SAME + (".editDistances",):
        assert b[suf] == a[suf], suf
    at_a, at_b = bai_ref.header_end(a[".sorted.bam"])[1], bai_ref.header_end(b[".sorted.bam"])[1]
    assert a[".sorted.bam"][:at_a] == b[".sorted.bam"][:at_b]
    ra, rb = bam_ref.decode_records(a[".sorted.bam"][at_a:]), bam_ref.decode_records(b[".sorted.bam"][at_b:])
    assert len(ra) == len(rb) >= 20
    assert any(r["qual"] != b"\xff" * r["l_seq"] for r in ra)       # (the qualities did reach the run with every output)
    for x, y in zip(ra, rb):
        assert y["qual"] == b"\xff" * y["l_seq"] and dict(x, qual=y["qual"]) == y, x["name"]


@pytest.mark.parametrize("tag", ["all", "sorted"])
def test_the_index_of_the_sorted_bam(runs, tag):
    """the index holds compressed offsets, which move with the QUAL bytes: each run's is held to the restatement on the run's own file as it was written"""
    run = runs["as written"][tag]
    assert run[".sorted.bam.bai"] == bai_ref.build(run[".sorted.bam"])


def test_the_read_files_alone(runs):
    a, b = runs["all"], runs["extract"]
    assert sorted(b) == sorted(list(SAME) + [".unmapped.fa.gz", ".mapped.fa.gz"])
    for suf in SAME:
        assert b[suf] == a[suf], suf
    for which in (".unmapped", ".mapped"):
        fastq = a[which + ".fq.gz"].split(b"\n")
        assert len(fastq) % 4 == 1 and len(fastq) > 4
        assert b[which + ".fa.gz"] == b"".join(b">" + fastq[i][1:] + b"\n" + fastq[i + 1] + b"\n" for i in range(0, len(fastq) - 1, 4)), which
