"""The definition of mapDirectly --consensus (metamaps_amd/csrc/mm_cons_core.hpp), built for the host with g++ — plain, and as a stand-alone program under the
address and undefined-behaviour sanitizers — against the plain restatement tests/cons_ref.py: the built cases of tests/cons_cases.py (alleles at position 0 and
at the last base, the 2 / 2 tie, overlapping and abutting deletions, alleles on removed positions and on a deletion's anchor, two insertions at one anchor,
insertions of 24 and 25 bases, a deletion of 65 535, depth D and D - 1, reference bytes that are no base, consensus lengths around the line width, contigs
that are not written), 200 random tables over low-complexity contigs, every refusal, and the planted truth of tests/test_gpu_cli_vcf.py.  CPU."""
import os
import subprocess

import pytest

import cons_cases
import cons_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("cons_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_cons_core.cpp")], check=True, timeout=300)
    return p


def world_text(w):
    keys = w.get("order") or sorted(w["t"])
    return (f"W {w['D']} {w['F']!r} {w['C']!r} {w['width']} {len(w['contigs'])} {len(keys)} {len(w['iv'])}\n" + "".join("=" + c.decode("latin-1") + "\n" for c in w["contigs"])
            + "".join(f"{k[0]} {k[1]} {w['t'].get(k, 3)}\n" for k in keys) + "".join(f"{c} {a} {b}\n" for c, a, b in w["iv"]))


def run(exe, worlds):
    """per world None (refused) or {contig: (stats list, text bytes)}"""
    p = subprocess.run([exe], input="".join(world_text(w) for w in worlds).encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out, buf, at = [], p.stdout, 0
    cur = {}
    while at < len(buf):
        end = buf.index(b"\n", at)
        words = buf[at:end].split()
        at = end + 1
        if words[0] == b"R":
            out.append(None)
        elif words[0] == b"E":
            out.append(cur); cur = {}
        else:
            assert words[0] == b"C" and len(words) == 3 + len(cons_ref.STATS)
            n = int(words[-1])
            cur[int(words[1])] = ([int(x) for x in words[2:-1]], buf[at:at + n])
            at += n
    assert len(out) == len(worlds) and cur == {}
    return out


def expected(w):
    res = cons_ref.consensus(w["t"], w["iv"], w["contigs"], w["D"], w["F"], w["C"])
    return {c: ([s[k] for k in cons_ref.STATS], cons_ref.wrapped(text, w["width"]).encode() if text is not None else b"") for c, (s, text, _) in res.items()}


def test_built_cases(exe):
    w = cons_cases.built_world()
    want = expected(w)
    for width in (60, 1, 7):
        assert run(exe, [dict(w, width=width)])[0] == expected(dict(w, width=width)), width
    res = cons_ref.consensus(w["t"], w["iv"], w["contigs"], 3, 0.5, 0.0)   # the restatement itself, by hand
    c = {name: k for k, name in enumerate(cons_cases.CASES)}
    stats = lambda name: res[c[name]][0]
    text = lambda name: res[c[name]][1]
    ref = lambda name: w["contigs"][c[name]].decode("latin-1").upper()
    pick = lambda name, *keys: [stats(name)[k] for k in keys]
    assert pick("ends", "snvs", "insertions", "insertedBases", "dropped", "consensusLength") == [2, 2, 3, 0, 103]
    assert text("ends")[0] != ref("ends")[0] and text("ends")[1:3] == "GT" and text("ends")[-1] == "A" and text("ends")[-2] != ref("ends")[99]
    assert pick("del_to_end", "deletions", "deletedBases", "consensusLength") == [1, 4, 96] and text("del_to_end") == ref("del_to_end")[:96]
    assert pick("tie", "snvs", "dropped") == [1, 1] and text("tie")[50] == "C"
    assert pick("d123", "deletions", "deletedBases", "dropped") == [3, 11 + 5 + 3, 2]
    assert text("d123") == ref("d123")[:10] + ref("d123")[21:51] + ref("d123")[59:]
    assert pick("on_removed", "snvs", "deletions", "insertions", "insertedBases", "dropped") == [2, 1, 2, 7, 2]
    r = ref("on_removed")
    assert text("on_removed")[21:24] == "TTG" and text("on_removed")[20] != r[20] and text("on_removed")[24:27] == r[31:34]
    assert pick("two_ins", "insertions", "insertedBases", "dropped") == [1, 1, 1] and text("two_ins")[41] == "A"
    assert text("ins_24_25")[31:55] == "ACGTTGCA" * 3 and text("ins_24_25")[41 + 24:41 + 24 + 25] == "N" * 25
    assert pick("big", "deletions", "deletedBases", "insertions", "insertedBases") == [3, 65535 + 64 + 65, 3, 64 + 65 + 200]
    assert pick("depth", "called", "snvs", "dropped") == [41 + 11, 2, 0] and text("depth")[51] == "N" and text("depth")[81] == "N" and text("depth")[9] == "N" and text("depth")[10] != "N"
    assert text("ref_bytes")[20:24] == "NNNA"
    assert [len(want[c[f"len{n}"]][1]) for n in (59, 60, 61, 120)] == [60, 61, 63, 122]
    assert want[c["len61"]][1][59:63] == ref("len61")[59].encode() + b"\n" + ref("len61")[60].encode() + b"\n"
    assert want[c["straddle"]][1][58:64] == b"AC\nGTA" and text("straddle")[58:63] == "ACGTA"
    assert c["no_intervals"] not in res and pick("nothing_called", "called", "written", "consensusLength", "dropped") == [0, 0, 0, 0] and text("nothing_called") is None


def test_called_threshold(exe):
    w = cons_cases.called_world()
    got = run(exe, [w])[0]
    assert got == expected(w)
    assert [got[c][0][1:4] for c in (0, 1, 2)] == [[50, 1, 100], [50, 0, 0], [49, 0, 0]] and got[1][0][4] == 1 and got[1][1] == b""


def test_200_random_tables(exe):
    worlds = cons_cases.random_worlds()
    assert len(worlds) == 200
    got = run(exe, worlds)
    total = dict.fromkeys(cons_ref.STATS, 0)
    for k, (w, g) in enumerate(zip(worlds, got)):
        want = expected(w)
        assert g == want, k
        for s, _ in want.values():
            for name, x in zip(cons_ref.STATS, s):
                total[name] += x
    assert min(total[k] for k in ("snvs", "deletions", "insertions", "dropped")) > 100 and total["written"] > 100, total
    joined = [cons_cases.joined(worlds[k::len(cons_cases.COMBOS)]) for k in range(len(cons_cases.COMBOS))]
    assert run(exe, joined) == [expected(w) for w in joined]


def test_every_refusal(exe):
    good, bad = cons_cases.refused_worlds()
    got = run(exe, [good] + [w for _, w in bad] + [good])
    assert got[0] == expected(good) and got[-1] == got[0] and got[1:-1] == [None] * len(bad), [why for (why, _), g in zip(bad, got[1:-1]) if g is not None]


def test_the_planted_truth(exe):
    """the world of tests/test_gpu_cli_vcf.py at D = 3, F = 0.5, over the perfect alignments"""
    import vcf_ref
    from test_gpu_cli_vcf import planted, read_spans, truth_jobs
    ref, strain, segs, edits = planted()
    jobs = truth_jobs(ref, strain, segs, read_spans())
    iv = [vcf_ref.interval(j) for j in jobs]
    t = vcf_ref.table(jobs, [ref])
    s, text, col = cons_ref.consensus(t, iv, [ref], 3, 0.5, 0.0)[0]
    assert (s["snvs"], s["deletions"], s["insertions"], s["dropped"]) == (29, 6, 3, 0)
    assert sum(1 for kind, _ in edits.values() if kind == "X") == 30
    assert s["consensusLength"] == len(text) == 29_997 == len(strain) and len(ref) - s["called"] == 1_406
    assert all(a == "N" or a == chr(b) for a, b in zip(text, strain))
    w = dict(contigs=[ref], t=t, iv=iv, D=3, F=0.5, C=0.0, width=60)
    assert run(exe, [w])[0] == expected(w)
