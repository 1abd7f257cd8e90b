"""The definition of the base-modification counts (metamaps_amd/csrc/mm_mods_core.hpp), built for the host with g++ — plain, and as a stand-alone
program under the address and undefined-behaviour sanitizers — against the plain restatement tests/mods_ref.py on the cases of tests/mods_cases.py: the
plane of reads of 0 to 4 097 bases (calls on bases 0, 63, 64 and the last one, ordinals at and beyond the letter's count, the three modes, two groups on
one letter at every tie, an unlisted code, lower case and N, empty skip lists, skips whose sums pass 2^32), the events of = runs of 1 to 200 columns on
both strands under the thresholds 0, 204 and 255, every rule, and the rows of the finish.  CPU."""
import os
import subprocess

import pytest

import mods_cases
import mods_ref
import pileup_cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("mods_core") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", p, os.path.join(HERE, "test_mods_core.cpp")], check=True, timeout=300)
    return p


def run(exe, mode, text, n_lines):
    p = subprocess.run([exe, mode], input=text.encode("latin-1"), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = p.stdout.decode().splitlines()
    assert len(out) == n_lines
    return out


def plane_line(read, groups):
    gs = " ".join(f"{g['base']} {g['code']} {ord(g['mode']) if g['mode'] else 0} {len(g['skips'])} " + " ".join(str(int(x)) for x in list(g["skips"]) + list(g["ml"])) for g in groups)
    return f"={bytes(read).decode('latin-1')} {len(groups)} {gs}"


def want_plane(read, groups):
    try:
        who, prob = mods_ref.plane(read, groups)
    except mods_ref.DataError as e:
        return f"E {e.group}"
    return f"{who.hex()} {prob.hex()}"


def test_plane_cases(exe):
    cases = mods_cases.plane_cases()
    got = run(exe, "plane", "\n".join(plane_line(r, g) for _, r, g, _ in cases) + "\n", len(cases))
    for (name, read, groups, bad), g in zip(cases, got):
        assert g == want_plane(read, groups), name
        assert (g == f"E {bad}") == (bad is not None), name
    by = {name: (read, mods_ref.plane(read, groups)) for name, read, groups, bad in cases if bad is None}
    # the restatement itself, by hand
    read, (who, prob) = by["edges_4097"]
    assert [who[i] for i in (0, 63, 64, 4096)] == [3, 3, 3, 3] and [prob[i] for i in (0, 63, 64, 4096)] == [230, 223, 216, 209] and sum(1 for w in who if w) == 4
    read, (who, prob) = by["mode_."]
    cs = [i for i, ch in enumerate(read.upper()) if ch == ord("C")]
    assert {who[i] for i in cs} == {1, 3} and {prob[i] for i in cs} == {255, 250} and all(who[i] == 0 for i in range(len(read)) if i not in cs)
    assert by["mode_absent"][1] == by["mode_."][1] and {w for w in by["mode_?"][1][0]} == {0, 3}
    assert set(by["empty_skips_."][1][0]) == {0, 1} and set(by["empty_skips_?"][1][0]) == {0}
    named = lambda n: sorted({(w, p) for w, p in zip(*by[n][1]) if w})
    assert named("two_groups_sum_255") == [(4, 155)] and named("two_groups_sum_above_255") == [(3, 200)] and named("two_groups_tie_to_canonical") == [(1, 100)]
    assert named("two_groups_equal_p_first") == [(3, 120)] and named("two_groups_second_larger") == [(4, 200)]
    assert (2, 222) in named("unlisted_code") and (5, 255) in named("unlisted_code") and set(by["no_groups"][1][0]) == {0}
    assert {len(r) for _, r, _, _ in cases} >= set(mods_cases.LENGTHS)


def event_line(j, k, contigs, T, n_reads=None, **over):
    j = dict(j, **over)
    pl = "-" if j.get("plane") is None else ("".join("%02x%02x" % wp for wp in zip(*j["plane"])) or "-")
    return (f"{j.get('read_index', k)} {k + 1 if n_reads is None else n_reads} {j.get('contig_index', j['c'])} {len(contigs)} {j['strand']} {j['first']} {j['d']} {j.get('use', 1)} "
            f"{len(j['read'])} {len(contigs[j['c']])} {T} {pl} {len(j['runs'])} " + " ".join(str(int(w)) for w in j["runs"]))


def check_events(exe, contigs, jobs, T, names=None):
    got = run(exe, "events", "\n".join(event_line(j, k, contigs, T) for k, j in enumerate(jobs)) + "\n", len(jobs))
    for k, (g, j) in enumerate(zip(got, jobs)):
        want = sorted(mods_ref.key(*e) for e in mods_ref.events(j, T)) if mods_ref.contributes(j) else []
        assert g == (" ".join(str(x) for x in want) if want else "-"), (k, names[k] if names else None, T)
    return got


@pytest.mark.parametrize("T", [0, 204, 255])
def test_event_cases(exe, T):
    contigs, jobs = mods_cases.event_world()
    got = dict(zip(jobs, check_events(exe, contigs, list(jobs.values()), T, list(jobs))))
    for name in ("no_eq", "not_used", "not_aligned", "no_plane"):
        assert got[name] == "-", name
    classes = {int(x) & 7 for n in ("fwd", "rev") for x in got[n].split()}
    assert classes == {0, 2, 3, 4, 5} if T == 0 else classes >= {0, 1, 2, 3, 5} and (T == 255 or 4 in classes)   # (C+h reaches 255 on few bases)
    assert {int(x) >> 3 & 1 for x in got["fwd"].split()} == {0} and {int(x) >> 3 & 1 for x in got["rev"].split()} == {1}
    # prob == T - 1 fails and prob == T passes: the stored bytes hold both sides of both thresholds
    probs = {p for j in jobs.values() if j["plane"] for w, p in zip(*j["plane"]) if w}
    assert {203, 204, 254, 255} <= probs
    assert got["one_base"] == "-" or len(got["one_base"].split()) == 1


def test_random_jobs(exe):
    contigs, jobs = mods_cases.random_world()
    got = check_events(exe, contigs, jobs, mods_ref.DEFAULT_MIN_ML)
    keys = [int(x) for g in got if g != "-" for x in g.split()]
    assert {(k >> 3 & 1, k & 7) for k in keys} == {(s, c) for s in (0, 1) for c in range(6)} and len(keys) > 5000


def test_every_rule(exe):
    contigs, _ = pileup_cases.built_world()
    cases = pileup_cases.broken_jobs(contigs)
    lines = []
    for j, over, rule in cases:
        over = dict(over)
        idx = {k + "_index": over.pop(k) for k in ("read", "contig") if k in over}
        plane = (bytes([1]) * len(j["read"]), bytes([255]) * len(j["read"]))
        lines.append(event_line(dict(j, plane=plane, **idx), 0, contigs, 204, 1, **over))
    assert run(exe, "events", "\n".join(lines) + "\n", len(lines)) == [f"E {rule}" for _, _, rule in cases]
    assert sorted({rule for _, _, rule in cases}) == [1, 2, 4, 5, 6]


@pytest.mark.parametrize("world", mods_cases.row_worlds(), ids=lambda w: w[0])
def test_rows(exe, world):
    name, contigs, t, code_base, min_cov = world
    want = mods_ref.rows(t, contigs, code_base, min_cov)
    keys = sorted(t)
    text = f"{min_cov} {code_base} {len(keys)}\n" + "".join(f"{k} {t[k]} {contigs[mods_ref.unkey(k)[0]][mods_ref.unkey(k)[1]]}\n" for k in keys)
    got = run(exe, "rows", text, len(want))
    assert got == [f"{mods_ref.key(c, pos, s, k)} {a} {b} {o} {f}" for c, pos, s, k, a, b, o, f in want]
    if name == "all":                                              # the restatement itself, by hand
        at = {(c, pos, s, k): (a, b, o, f) for c, pos, s, k, a, b, o, f in want}
        assert at[(1, 0, 1, 0)] == (2, 1, 3, 0) and at[(1, 0, 1, 1)] == (3, 1, 2, 0)      # each one's N_other holds the other
        assert not any(c == 1 and pos in (1, 2) for c, pos, _, _ in at)                    # fail calls only; no code of base T
        assert at[(1, 5, -1, 2)] == (4, 1, 0, 0) and at[(1, 4, -1, 0)] == (0xFFFFFFFF, 0, 0xFFFFFFFF + 7, 0)
        assert not any(c == 0 and pos in (4, 9) for c, pos, _, _ in at)                    # N and R
        assert (0, 5, 1, 2) in at and (0, 5, -1, 2) not in at and (0, 8, -1, 2) in at      # lower-case a; t on the - strand is A
    if name == "coverage_eq_min":
        assert [(c, pos, k) for c, pos, _, k, *_ in want] == [(1, 0, 0), (1, 0, 1)]         # coverage 3 kept, 2 not
