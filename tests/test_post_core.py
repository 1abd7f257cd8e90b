"""The arithmetic of K8 and of K9's set-up and stop rule (metamaps_amd/csrc/mm_post_core.hpp), built for the host with g++ — plain, and as a
stand-alone program under the address and undefined-behaviour sanitizers: parse6 against the text round trip it restates (in the C++ program:
snprintf("%g") then strtod), dev_binom_pmf against the exact binomial mass (mpmath), mapq_success_p and em_stop_now against their float64
restatements (tests/post_ref.py).  CPU."""
import math
import os
import struct
import subprocess

import mpmath
import numpy as np
import pytest

import post_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def unbits(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("post") / "t")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread"] + flags + ["-o", p, os.path.join(HERE, "test_post_core.cpp")], check=True, timeout=300)
    return p


def ask(exe, lines):
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = [int(x) for x in p.stdout.decode().split()]
    assert len(out) == len(lines)
    return out


def test_parse6_is_the_text_round_trip(exe):
    """every six-digit mantissa of every decade of [1e-17, 1e22) and one in 97 up to 1e28, neighbours, ties (exact ones and the doubles nearest to
    inexact ones), the carry, the powers of ten, 10^7 random values, the identities K8 feeds it: the bits of strtod("%g").  Below 1e-17 down
    to the denormals and from 1e28 up: finite, 0 for a denormal text, the same six digits, within 4 * 2^-53.  The walk is in test_post_core.cpp."""
    p = subprocess.run([exe, "parse6"], capture_output=True, timeout=900)
    assert p.returncode == 0, p.stdout.decode()[-4000:] + p.stderr.decode()[-2000:]
    assert " 0 failures" in p.stdout.decode()


def test_emhost_parse6_is_the_same_round_trip(exe):
    """metamaps_amd.emhost.parse6 is the text round trip itself: equal to parse6 to the bit from 1e-17 up, finite and within 4 * 2^-53 below,
    0 for denormal texts, on the five values at which the arithmetic of the parent overflowed and on random ones"""
    from metamaps_amd import emhost
    rng = np.random.default_rng(7)
    v = np.concatenate([[9.99e-304, 3e-305, 3e-308, 2.3e-308, 5e-320, post_ref.DBL_MIN, 0.0, 1.0, 0.5, 1e-17], 10.0 ** rng.uniform(-17, 0, 2000), 10.0 ** rng.uniform(-320, -17, 2000)])
    host = emhost.parse6(v)
    core = np.array([unbits(b) for b in ask(exe, [f"6 {bits(x)}" for x in v])])
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(core))
    assert host[:7].tolist() == [9.99e-304, 3e-305, 3e-308, 2.3e-308, 0.0, 0.0, 0.0]
    big = v >= 1e-17
    assert np.array_equal(host[big], core[big])
    assert np.array_equal(host == 0, core == 0)
    nz = host != 0
    assert np.all(np.abs(core[nz] - host[nz]) <= 4 * 2.0 ** -53 * host[nz])
    assert ["%g" % x for x in core[nz]] == ["%g" % x for x in v[nz]]


N_GRID = [1, 2, 17, 250, 2_222, 12_000, 32_768, 60_000]
IDENTITIES = [0.80, 0.8812, 0.95, 0.9899]


def pmf_cases():
    rng = np.random.default_rng(2026)
    cases = []
    for n in N_GRID:
        lens = [1_000, 10_000] + ([int(4.5 * n)] if int(4.5 * n) >= 32 else [])          # (4.5 n bases hold n minimizers; below 2 k there are no k-mers)
        ps = sorted({post_ref.success_p(i, L, 16) for i in IDENTITIES for L in lens} | {0.0, 1.0})
        for p in ps:
            mode = int(math.floor((n + 1) * p))
            ks = {0, 1, n - 1, n, mode - 1, mode, mode + 1} | set(int(x) for x in rng.integers(0, n + 1, 40))
            cases += [(n, p, k) for k in sorted(ks) if 0 <= k <= n]
    return cases


def test_success_p_is_its_float64_restatement(exe):
    q = [(i, L, k) for i in IDENTITIES + [0.0, 1.0, 0.5, 0.999999] for L in (1_000, 1_001, 10_000, 54_000, 270_000) for k in (15, 16)]
    got = ask(exe, [f"P {bits(i)} {L} {k}" for i, L, k in q])
    assert got == [bits(post_ref.success_p(*x)) for x in q]
    assert post_ref.success_p(1.0, 10_000, 16) == 1.0 and post_ref.success_p(0.0, 1_000, 16) == 0.0     # the two ends K8's special cases rest on


def test_binom_pmf_against_exact_mass(exe):
    """the error of the lgamma formula against the exact mass of the double p, in units of S * 2^-52 (post_ref.pmf_scale): at most PMF_C_HOST"""
    cases = pmf_cases()
    got = [unbits(b) for b in ask(exe, [f"B {n} {bits(p)} {k}" for n, p, k in cases])]
    worst, worst_at, n_rel = 0.0, None, 0
    for (n, p, k), g in zip(cases, got):
        want = post_ref.pmf_exact(n, p, k)
        S = post_ref.pmf_scale(n, p, k)
        if S == 0:
            assert g == float(want) and g in (0.0, 1.0), (n, p, k, g)
            continue
        assert math.isfinite(g) and g >= 0
        if want < mpmath.mpf("1e-290"):                            # the denormal range of exp: absolutely as well
            assert abs(g - float(want)) <= 1e-300 + float(want) * post_ref.PMF_C_HOST * S * post_ref.ULP, (n, p, k, g, float(want))
            continue
        ratio = float(abs(mpmath.mpf(g) - want) / want) / (S * post_ref.ULP)
        n_rel += 1
        if ratio > worst:
            worst, worst_at = ratio, (n, p, k)
    print(f"dev_binom_pmf on the host: worst err / (S * 2^-52) = {worst:.4f} at (n, p, k) = {worst_at}, {n_rel} masses above 1e-290 of {len(cases)} cases")
    assert n_rel > 1000
    assert worst <= post_ref.PMF_C_HOST, (worst, worst_at)


def test_stop_rule_at_its_thresholds(exe):
    """em_stop_now on both sides of gain == 1 and of 1 - ll / ll_prev == 1e-4, double by double, and on the first iteration"""
    q = []
    for ll_prev, ll in ((-1e6, -999_999.0), (-5_000.0, -4_999.5), (-20_000.0, -19_998.0), (-3.0, -2.9997), (5_000.0, 5_000.5), (-1e6, -1e6)):
        x = ll
        for _ in range(8):
            x = math.nextafter(x, -math.inf)
        for _ in range(17):
            q += [(it, x, ll_prev) for it in (0, 1, 7)]
            x = math.nextafter(x, math.inf)
    got = ask(exe, [f"S {it} {bits(ll)} {bits(lp)}" for it, ll, lp in q])
    want = [int(post_ref.stop_now(*x)) for x in q]
    assert got == want
    assert all(g == 0 for g, x in zip(got, q) if x[0] == 0)
    gain = [g for g, x in zip(got, q) if x[0] == 1 and x[2] == -1e6 and abs(x[1] + 999_999.0) < 1e-6]
    rel = [g for g, x in zip(got, q) if x[0] == 1 and x[2] == -5_000.0]
    assert set(gain) == {0, 1} and set(rel) == {0, 1}               # the walk crosses each threshold
    assert post_ref.stop_now(1, -999_999.0, -1e6) and not post_ref.stop_now(1, math.nextafter(-999_999.0, 0.0), -1e6)      # gain == 1 stops, the next double does not
