"""`classify --min-identity T [--refit]` and `mapDirectly --then-classify ... --min-identity T --refit`: PREFIX.extractedIdentities and PREFIX.EM-filtered* beside
unchanged outputs, recomputed byte for byte in Python from PREFIX, PREFIX.EM, PREFIX.EM.WIMP, PREFIX.EM.reads2Taxon and the DB's taxonomy (tests/ident_ref.py);
the refit against an EM the test runs itself on the filtered problem; the same files from two logical devices and through --then-classify; the refusals.
T is chosen from the data: the midpoint of the widest gap between the genomes' median identities that leaves three genomes on either side."""
import os
import re
import subprocess

import numpy as np
import pytest

import ident_ref
from test_gpu_cli import CLI
from test_gpu_cli_bootstrap import OUTS, _copy_mappings

pytestmark = pytest.mark.gpu
FILTERED = [".extractedIdentities", ".EM-filtered", ".EM-filtered.reads2Taxon", ".EM-filtered.WIMP"]
REFIT = [".EM-filtered.refit", ".EM-filtered.refit.reads2Taxon", ".EM-filtered.refit.WIMP"]
FILTER_LINE = re.compile(r"^Identity filter: threshold (\S+), median identity (\S+), (\d+) of (\d+) best identities at or below it, (\d+) of (\d+) genomes removed, "
                         r"(\d+) reads set to unclassified$", re.M)
REFIT_LINE = re.compile(r"^Refit: (\d+) reads, (\d+) mappings, (\d+) reads lost every mapping, (\d+) EM iterations$", re.M)


def _run(args):
    return subprocess.run([CLI] + args, capture_output=True, timeout=900)


def _classify(run, tag, extra):
    dst = str(run["dir"] / tag)
    _copy_mappings(run["m"], dst)
    p = _run(["classify", "--DB", run["db"].dir, "--mappings", dst, "--minreads", "3"] + extra)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dst, p.stdout.decode()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from metamaps_amd import synth
    d = tmp_path_factory.mktemp("identf")
    db = synth.make_db(str(d / "db"), n_genomes=40, genome_len=30_000, seed=7)     # (its 3 % pairs: reads map to two genomes)
    rd = synth.make_reads(db, str(d / "r.fq"), n_reads=2000, read_len=3000, seed=3, abundance_sigma=0.5)
    out = {"dir": d, "db": db, "q": rd["path"], "m": str(d / "map0")}
    p = _run(["mapDirectly", "--all", "-r", db.fasta, "-q", rd["path"], "-o", out["m"]])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out["plain"], _ = _classify(out, "plain", [])
    # T from the data
    _, n0 = ident_ref.recompute(out["plain"], db.dir, 0.0)
    med = sorted(n0["medians"].values())
    assert len(med) >= 6
    k = max(range(2, len(med) - 3), key=lambda k: med[k + 1] - med[k])
    mid = "%.6f" % ((med[k] + med[k + 1]) / 2)
    assert med[k] < float(mid) < med[k + 1]
    whole, frac = mid.split(".")
    out["T_text"] = "0." + whole.rjust(2, "0") + frac               # the midpoint divided by 100, digit for digit
    assert len(whole) <= 2
    out["T"] = float(out["T_text"])
    out["files"], out["n"] = ident_ref.recompute(out["plain"], db.dir, out["T"], refit=True)
    n = out["n"]
    assert n["genomes_removed"] >= 3 and n["genomes"] - n["genomes_removed"] >= 3 and n["reads_removed"] >= 20
    assert any(n["taxon"][r] in n["removed"] and kept for r, kept in enumerate(n["kept"]))   # a removed read with an entry in a genome that stays
    out["filtered"], out["stdout_filtered"] = _classify(out, "filtered", ["--min-identity", out["T_text"]])
    out["refit"], out["stdout_refit"] = _classify(out, "refit", ["--min-identity", out["T_text"], "--refit"])
    return out


def _same_old_outputs(a, b):
    for suf in OUTS:
        assert os.path.exists(a + suf) == os.path.exists(b + suf), suf
        if os.path.exists(a + suf):
            assert open(a + suf, "rb").read() == open(b + suf, "rb").read(), suf
    assert os.path.exists(a + ".EM") and os.path.exists(a + ".EM.WIMP")


def _read(path):
    with open(path) as f:
        return f.read()


def test_no_new_file_without_the_flags(run):
    again, _ = _classify(run, "again", [])
    _same_old_outputs(run["plain"], again)
    for suf in FILTERED + REFIT:
        assert not os.path.exists(run["plain"] + suf) and not os.path.exists(again + suf), suf


def test_filtered_files_equal_the_text_level_restatement(run):
    _same_old_outputs(run["plain"], run["filtered"])
    for suf in FILTERED:
        assert _read(run["filtered"] + suf) == run["files"][suf], suf
    for suf in REFIT:
        assert not os.path.exists(run["filtered"] + suf), suf
    m, n = FILTER_LINE.search(run["stdout_filtered"]), run["n"]
    assert m, run["stdout_filtered"][-1000:]
    assert m.group(1) == "%g" % n["thr"] and m.group(2) == "%g" % n["median_all"]
    assert [int(x) for x in m.groups()[2:]] == [n["n_le"], n["n"], n["genomes_removed"], n["genomes"], n["reads_removed"]]
    assert not REFIT_LINE.search(run["stdout_filtered"])


@pytest.fixture(scope="module")
def own_em(run):
    """the EM of the filtered problem, run by the test: the problem of the plain run, the removed genomes' entries dropped, mm_em_run from 1 / n_taxa"""
    from metamaps_amd import capi, emhost
    P = emhost.load_problem(run["plain"], run["db"].dir)
    keep = ~np.isin(P.taxon, [i for i, t in enumerate(P.taxa) if t in run["n"]["removed"]])
    per = np.add.reduceat(keep.astype(np.int64), P.read_off[:-1])
    off = np.concatenate([[0], np.cumsum(per[per > 0])])
    ctx = capi.Context(0)
    em = ctx.em(off, P.taxon[keep], P.mapq[keep], P.inv_nloc[keep], len(P.taxa))
    f, ll = em.run(np.full(len(P.taxa), 1.0 / len(P.taxa)), max_iter=1024)
    post, best = em.posteriors(f)
    em.close(); ctx.close()
    read_ids = [P.read_ids[r] for r in np.flatnonzero(per > 0)]
    lost = [P.read_ids[r] for r in np.flatnonzero(per == 0)]
    return dict(P=P, off=off, taxon=P.taxon[keep], f=f, rounds=len(ll), post=post, best=best, read_ids=read_ids, lost=lost)


def test_refit_against_an_em_run_by_the_test(run, own_em):
    _same_old_outputs(run["plain"], run["refit"])
    for suf in FILTERED:
        assert _read(run["refit"] + suf) == run["files"][suf], suf
    n, E = run["n"], own_em
    lines = _read(run["refit"] + ".EM-filtered.refit").splitlines()
    assert "".join(ln.rsplit(" ", 1)[0] + "\n" for ln in lines) == run["files"][".EM-filtered.refit"]      # the kept lines, byte for byte
    got_post = np.array([float(ln.rsplit(" ", 1)[1]) for ln in lines])
    assert len(got_post) == len(E["post"]) == n["kept_entries"]
    worst = float(np.max(np.abs(got_post - E["post"])))
    print("largest posterior difference", worst)
    assert worst <= 1e-5                                            # (the README's contract for EM results; six printed decimals: 5e-7)
    m = REFIT_LINE.search(run["stdout_refit"])
    assert m and [int(x) for x in m.groups()] == [n["kept_reads"], n["kept_entries"], n["lost"], E["rounds"]], run["stdout_refit"][-500:]
    # reads2Taxon: the arg-max of those posteriors, lost reads at 0, then the unmapped reads as in .EM.reads2Taxon
    taxa = E["P"].taxa
    new = {rid: taxa[E["taxon"][b]] for rid, b in zip(E["read_ids"], E["best"])}
    new.update({rid: "0" for rid in E["lost"]})
    old = [ln.split("\t") for ln in _read(run["plain"] + ".EM.reads2Taxon").splitlines()]
    want = "".join(rid + "\t" + (new[rid] if k < n["n"] else t) + "\n" for k, (rid, t) in enumerate(old))
    assert _read(run["refit"] + ".EM-filtered.refit.reads2Taxon") == want
    # the WIMP: frequencies through cleanF with the kept reads as ReadsMapped; the count rows
    wimp = [ln.split("\t") for ln in _read(run["refit"] + ".EM-filtered.refit.WIMP").splitlines()[1:]]
    reads_per = {}
    for t in new.values():
        reads_per[t] = reads_per.get(t, 0) + 1
    min_f = 0.9 / n["kept_reads"]
    f = {t: v for t, v in zip(taxa, E["f"]) if not (v < min_f and t not in reads_per)}
    total = sum(f.values())
    rows = {r[1]: r for r in wimp if r[0] == "definedGenomes" and r[1] not in ("0", "-3")}
    assert set(rows) == set(f) and not set(rows) & n["removed"]
    worst = max(abs(float(rows[t][4]) - f[t] / total) for t in f)
    print("largest frequency difference", worst)
    assert worst <= 1e-5
    assert all(int(rows[t][3]) == reads_per.get(t, 0) for t in rows)
    old_w = [ln.split("\t") for ln in _read(run["plain"] + ".EM.WIMP").splitlines()[1:]]
    count = lambda w, name: {int(r[3]) for r in w if r[1] == "-3" and r[2] == name}
    assert count(wimp, "totalReads") == count(old_w, "totalReads") and count(wimp, "readsLongEnough") == count(old_w, "readsLongEnough")
    (u_old,), (u_new,) = count(old_w, "readsLongEnough_unmapped"), count(wimp, "readsLongEnough_unmapped")
    assert u_new == u_old + n["lost"] and n["lost"] > 0


def test_two_logical_devices_and_then_classify_write_the_same_files(run):
    two, _ = _classify(run, "two", ["--min-identity", run["T_text"], "--refit", "--devices", "0,0", "--em-host-reduce"])   # the filter: first device, all reads; the refit: both
    o = str(run["dir"] / "direct")
    p = _run(["mapDirectly", "--all", "-r", run["db"].fasta, "-q", run["q"], "-o", o, "--then-classify", run["db"].dir, "--minreads", "3",
              "--min-identity", run["T_text"], "--refit"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for other in (two, o):
        _same_old_outputs(run["plain"], other)
        for suf in FILTERED + REFIT:
            assert open(other + suf, "rb").read() == open(run["refit"] + suf, "rb").read(), (other, suf)


@pytest.mark.parametrize("args,word", [(["classify", "--refit"], "--refit"), (["classify", "--min-identity", "1.5"], "--min-identity"),
                                       (["classify", "--min-identity", "-0.1"], "--min-identity"), (["classify", "--min-identity", "abc"], "--min-identity"),
                                       (["index", "--min-identity", "0.8"], "--min-identity"), (["index", "--min-identity", "0.8", "--refit"], "--refit"),
                                       (["mapAgainstIndex", "--min-identity", "0.8"], "--min-identity"), (["mapAgainstIndex", "--min-identity", "0.8", "--refit"], "--refit")])
def test_refused_forms_of_the_flags(run, args, word):
    rest = {"classify": ["--DB", run["db"].dir, "--mappings", str(run["dir"] / "refused")],
            "index": ["-r", run["db"].fasta, "-i", str(run["dir"] / "idx")],
            "mapAgainstIndex": ["-i", str(run["dir"] / "idx"), "-q", run["q"], "-o", str(run["dir"] / "mai")]}[args[0]]
    if args[0] == "classify":
        _copy_mappings(run["m"], str(run["dir"] / "refused"))
    p = _run(args[:1] + rest + args[1:])
    assert p.returncode != 0 and word.encode() in p.stderr, p.stderr[-500:]
    if args[0] == "classify" and len(args) > 2:
        assert args[2].encode() in p.stderr                         # the value is named
    assert not os.path.exists(str(run["dir"] / "refused") + ".EM") and not os.path.exists(str(run["dir"] / "idx")) and not os.path.exists(str(run["dir"] / "mai"))


def test_thresholds_0_and_1(run):
    zero, _ = _classify(run, "zero", ["--min-identity", "0"])
    assert _read(zero + ".EM-filtered.reads2Taxon") == _read(zero + ".EM.reads2Taxon")
    one, text = _classify(run, "one", ["--min-identity", "1", "--refit"])
    n = run["n"]["n"]
    r2t = [ln.split("\t") for ln in _read(one + ".EM-filtered.reads2Taxon").splitlines()]
    assert len(r2t) > n and all(t == "0" for _, t in r2t)
    assert _read(one + ".EM-filtered") == "" and _read(one + ".EM-filtered.refit") == ""
    assert _read(one + ".EM-filtered.refit.reads2Taxon") == _read(one + ".EM-filtered.reads2Taxon")
    assert _read(one + ".EM-filtered.refit.WIMP").splitlines()[1:] == []          # no genome is left: the header alone
    m = REFIT_LINE.search(text)
    assert m and [int(x) for x in m.groups()] == [0, 0, n, 0]
