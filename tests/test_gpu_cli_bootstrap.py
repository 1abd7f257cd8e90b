"""`classify --bootstrap B [--bootstrap-seed S]`: PREFIX.EM.WIMP.bootstrap beside unchanged outputs, independent of the devices and of the
run, the same through `mapDirectly --then-classify`, strict flag values, intervals of the size binomial sampling predicts, and replicates
that drew no read (a sample of three mapped reads) left out of the statistics."""
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_cli import CLI

pytestmark = pytest.mark.gpu
OUTS = (".EM", ".EM.WIMP", ".EM.reads2Taxon", ".EM.reads2Taxon.krona", ".EM.contigCoverage", ".EM.lengthAndIdentitiesPerMappingUnit",
        ".EM.evidenceUnknownSpecies")


def _run(args, env=None):
    p = subprocess.run([CLI] + args, capture_output=True, timeout=900, env=dict(os.environ, **(env or {})))
    return p


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("boot")
    # genome pairs far apart and even abundances: most taxa get reads that map to them alone (the binomial check below)
    db = synth.make_db(str(d / "db"), n_genomes=10, genome_len=60_000, seed=7, pair_divergence=0.3, with_oddities=False)
    r1 = synth.make_reads(db, str(d / "r1.fq"), n_reads=260, read_len=3000, seed=3, abundance_sigma=0.3, with_oddities=False)
    r4 = synth.make_reads(db, str(d / "r4.fq"), n_reads=1040, read_len=3000, seed=3, abundance_sigma=0.3, with_oddities=False)
    out = {"dir": d, "db": db, "q1": r1["path"], "q4": r4["path"]}
    for tag, q in (("m1", r1["path"]), ("m4", r4["path"])):
        p = _run(["mapDirectly", "--all", "-r", db.fasta, "-q", q, "-o", str(d / tag)])
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out[tag] = str(d / tag)
    return out


def _copy_mappings(src, dst):
    for f in glob.glob(src + "*"):
        suf = f[len(src):]
        if suf.startswith(".EM"):
            continue
        with open(f, "rb") as a, open(dst + suf, "wb") as b:
            b.write(a.read())


def _classify(run, src, tag, extra):
    dst = str(run["dir"] / tag)
    _copy_mappings(src, dst)
    p = _run(["classify", "--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"] + extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dst, p.stdout.decode()


def _table(fn):
    lines = open(fn).read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def test_outputs_unchanged_and_rows_match_the_wimp(run):
    plain, _ = _classify(run, run["m1"], "plain", [])
    assert not os.path.exists(plain + ".EM.WIMP.bootstrap")
    boot, log = _classify(run, run["m1"], "boot", ["--bootstrap", "64", "--bootstrap-seed", "7"])
    assert re.search(r"Bootstrap: 64 replicates, seed 7, \d+-\d+ EM iterations", log), log[-2000:]
    for suf in OUTS:
        if os.path.exists(plain + suf) or os.path.exists(boot + suf):
            assert open(plain + suf, "rb").read() == open(boot + suf, "rb").read(), suf
    hdr, rows = _table(boot + ".EM.WIMP.bootstrap")
    assert hdr == ["AnalysisLevel", "taxonID", "Name", "EMFrequency", "BootstrapMean", "BootstrapSD", "Lower95", "Upper95"]
    _, wimp = _table(boot + ".EM.WIMP")
    want = [w[:3] + [w[4]] for w in wimp if w[1] != "-3"]
    assert [r[:4] for r in rows] == want
    assert any(r[2] == "Unclassified" for r in rows)
    for r in rows:
        mean, sd, lo, hi = map(float, r[4:])
        assert sd >= 0 and lo <= hi
        assert lo - 1e-6 * abs(lo) <= mean <= hi + 1e-6 * abs(hi), r


def test_same_file_for_any_devices_run_and_path(run):
    extra = ["--bootstrap", "40", "--bootstrap-seed", "3"]
    a, _ = _classify(run, run["m1"], "d0", extra + ["--devices", "0"])
    b, _ = _classify(run, run["m1"], "d000", extra + ["--devices", "0,0,0", "--em-host-reduce"])
    c, _ = _classify(run, run["m1"], "d0again", extra + ["--devices", "0"])
    ref = open(a + ".EM.WIMP.bootstrap", "rb").read()
    assert open(b + ".EM.WIMP.bootstrap", "rb").read() == ref
    assert open(c + ".EM.WIMP.bootstrap", "rb").read() == ref
    o = str(run["dir"] / "direct")
    p = _run(["mapDirectly", "--all", "-r", run["db"].fasta, "-q", run["q1"], "-o", o, "--then-classify", run["db"].dir, "--minreads", "3"] + extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(o + ".EM.WIMP.bootstrap", "rb").read() == ref
    d, _ = _classify(run, run["m1"], "seed4", ["--bootstrap", "40", "--bootstrap-seed", "4"])
    assert open(d + ".EM.WIMP.bootstrap", "rb").read() != ref


def test_replicates_without_a_read_are_left_out(run):
    """three mapped reads: e^-3 of the replicates draw none of them; their f is no estimate (mm_em_bootstrap: n_iter == 0) and must reach
    neither mean nor SD nor quantiles — once it made a whole row NaN"""
    from test_boot_core import weights_np
    n_keep, B, seed = 3, 64, 7
    src = run["m1"]
    dst = str(run["dir"] / "three")
    _copy_mappings(src, dst)
    ids, kept = [], []
    for ln in open(src):
        rid = ln.split(" ")[0]
        if rid not in ids:
            if len(ids) == n_keep:
                break
            ids.append(rid)
        kept.append(ln)
    assert len(ids) == n_keep <= 4
    with open(dst, "w") as o:
        o.write("".join(kept))
    meta = dict(ln.split() for ln in open(src + ".meta").read().splitlines() if ln.strip())
    meta["TotalReads"] = str(int(meta["TotalReads"]) - int(meta["ReadsMapped"]) + n_keep)
    meta["ReadsMapped"] = str(n_keep)
    with open(dst + ".meta", "w") as o:
        o.write("".join(f"{k} {v}\n" for k, v in meta.items()))
    w = weights_np(np.uint64(seed), np.arange(B, dtype=np.uint64)[:, None], np.arange(n_keep, dtype=np.uint64)[None, :]).reshape(B, n_keep)
    n_empty = int(np.count_nonzero(~w.any(axis=1)))
    assert 1 <= n_empty <= B - 2
    files = {}
    for tag, devices in (("three_d0", ["0"]), ("three_d00", ["0,0", "--em-host-reduce"])):      # (one device twice: no collective between the two)
        out = str(run["dir"] / tag)
        _copy_mappings(dst, out)
        p = _run(["classify", "--DB", run["db"].dir, "--mappings", out, "--minreads", "3", "--bootstrap", str(B), "--bootstrap-seed", str(seed), "--devices"] + devices)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        log = p.stdout.decode()
        m = re.search(r"Bootstrap: 64 replicates, seed 7, (\d+)-(\d+) EM iterations per replicate, .*, (\d+) of 64 drew no read and are left out", log)
        assert m, log[-2000:]
        assert int(m.group(3)) == n_empty and 1 <= int(m.group(1)) <= int(m.group(2)) < 10_000
        assert b"EM iterations without meeting the stop rule" not in p.stderr
        files[tag] = open(out + ".EM.WIMP.bootstrap", "rb").read()
    assert files["three_d0"] == files["three_d00"]
    _, rows = _table(str(run["dir"] / "three_d0") + ".EM.WIMP.bootstrap")
    assert rows
    for r in rows:
        assert all(re.fullmatch(r"[0-9.e+-]+", x) and math.isfinite(float(x)) for x in r[3:]), r       # no nan, no inf
        mean, sd, lo, hi = map(float, r[4:])
        assert sd >= 0 and lo <= mean <= hi, r


@pytest.mark.parametrize("bad", [["--bootstrap", "1"], ["--bootstrap", "100001"], ["--bootstrap", "x"], ["--bootstrap", "-5"], ["--bootstrap", "2.5"],
                                 ["--bootstrap", "10", "--bootstrap-seed", "-1"], ["--bootstrap", "10", "--bootstrap-seed", "18446744073709551616"],
                                 ["--bootstrap", "10", "--bootstrap-seed", "abc"]])
def test_bad_values_die(run, bad):
    dst = str(run["dir"] / "bad")
    _copy_mappings(run["m1"], dst)
    p = _run(["classify", "--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"] + bad)
    assert p.returncode != 0
    assert b"bootstrap" in p.stderr
    assert not os.path.exists(dst + ".EM.WIMP.bootstrap")


def _taxon_of_contig(c):
    return re.search(r"taxid\|(x?\d+)", c).group(1)


def _single_taxon_counts(prefix):
    """per taxon: reads whose mappings are all on that taxon, and whether every read that maps to it does so"""
    per_read = {}
    for ln in open(prefix):
        f = ln.split(" ")
        per_read.setdefault(f[0], set()).add(_taxon_of_contig(f[5]))
    n, clean = {}, {}
    for taxa in per_read.values():
        for t in taxa:
            n[t] = n.get(t, 0) + 1
            clean[t] = clean.get(t, True) and len(taxa) == 1
    return {t: n[t] for t in n if clean[t]}, len(per_read)


def test_intervals_have_the_binomial_width(run):
    widths = {}
    for tag in ("m1", "m4"):
        dst, _ = _classify(run, run[tag], tag + "_b200", ["--bootstrap", "200", "--bootstrap-seed", "11"])
        counts, n_mapped = _single_taxon_counts(run[tag])
        _, rows = _table(dst + ".EM.WIMP.bootstrap")
        got = {r[1]: r for r in rows if r[0] == "definedGenomes"}
        checked = 0
        for t, k in counts.items():
            if k < 20 or t not in got:
                continue
            widths.setdefault(t, {})[tag] = float(got[t][7]) - float(got[t][6])
            if k < 50:
                continue
            p = float(got[t][3])
            want = math.sqrt(p * (1 - p) / n_mapped)
            sd = float(got[t][5])
            assert 0.7 * want <= sd <= 1.4 * want, (tag, t, k, p, sd, want)
            checked += 1
        if tag == "m4":
            assert checked >= 1, (counts, sorted(got))
    ratios = [w["m1"] / w["m4"] for w in widths.values() if len(w) == 2]
    assert ratios
    assert 1.4 <= np.median(ratios) <= 2.8, ratios
