"""The bootstrap's counter-based Poisson(1) weights (metamaps_amd/csrc/mm_boot_core.hpp) against a numpy restatement of their
definition ("Bootstrap"), the pinned check values, and the Poisson(1) law."""
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
THRESHOLDS = np.array([3313563428353947, 6627126856707895, 8283908570884869, 8836169142277194, 8974234285125275, 9001847313694891,
                       9006449485123161, 9007106938184342, 9007189119816990, 9007198251109506, 9007199164238758, 9007199247250508,
                       9007199254168154, 9007199254700280, 9007199254738289, 9007199254740823], dtype=np.uint64)


def mix(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def weights_np(seed, r, i):
    seed, r, i = (np.asarray(a, dtype=np.uint64) for a in (seed, r, i))
    x = mix(seed ^ mix((r << np.uint64(32)) | i))
    u = x >> np.uint64(11)
    return (u[..., None] >= THRESHOLDS).sum(axis=-1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("boot") / "t")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", p, os.path.join(HERE, "test_boot_core.cpp")], check=True, timeout=300)
    return p


def weights_cpp(exe, seed, r, i):
    txt = "\n".join(f"{a} {b} {c}" for a, b, c in zip(seed.tolist(), r.tolist(), i.tolist())) + "\n"
    p = subprocess.run([exe], input=txt.encode(), capture_output=True, timeout=300, check=True)
    return np.frombuffer(p.stdout, dtype=np.uint8).astype(np.int64) - ord("a")


def test_thresholds_are_the_poisson_cdf():
    import decimal
    decimal.getcontext().prec = 60
    inv_e = 1 / decimal.Decimal(1).exp()
    acc, fact = decimal.Decimal(0), 1
    for k in range(16):
        fact *= max(k, 1)
        acc += inv_e / fact
        assert int((acc * (1 << 53)).to_integral_value(rounding=decimal.ROUND_FLOOR)) == int(THRESHOLDS[k])


def test_check_values():
    assert weights_np(1, 0, np.arange(8)).tolist() == [0, 2, 2, 3, 1, 2, 0, 0]
    assert weights_np(1, 1, np.arange(8)).tolist() == [0, 3, 0, 1, 1, 0, 2, 0]


def test_header_matches_numpy(exe):
    rng = np.random.default_rng(5)
    n = 1_000_000
    seed = rng.integers(0, 2**63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    r = rng.integers(0, 2**32, size=n, dtype=np.uint64)
    i = rng.integers(0, 2**32, size=n, dtype=np.uint64)
    r[:1000] = np.uint64(2**31) + np.arange(-500, 500, dtype=np.int64).astype(np.uint64)      # near 2^31
    i[1000:2000] = np.uint64(2**31) + np.arange(-500, 500, dtype=np.int64).astype(np.uint64)
    r[2000:3000] = 0; i[2000:3000] = np.arange(1000, dtype=np.uint64); seed[2000:3000] = 1
    got = weights_cpp(exe, seed, r, i)
    assert got.shape == (n,)
    assert np.array_equal(got, weights_np(seed, r, i))
    assert got[2000:2008].tolist() == [0, 2, 2, 3, 1, 2, 0, 0]


def test_poisson_law():
    n = 1_000_000
    w = weights_np(np.uint64(12345), np.arange(n) // 1000, np.arange(n) % 1000)
    assert abs(w.mean() - 1) < 0.01 and abs(w.var() - 1) < 0.01
    obs = np.bincount(w, minlength=8)
    p = np.array([math.exp(-1) / math.factorial(k) for k in range(7)])
    p = np.append(p, 1 - p.sum())                                 # 7 and more in one bin
    obs = np.append(obs[:7], obs[7:].sum())
    chi2 = (((obs - n * p) ** 2) / (n * p)).sum()
    assert chi2 < 24.3, (chi2, obs)                               # chi-square, 7 degrees of freedom, p = 0.001
