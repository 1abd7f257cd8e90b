"""mm_depth_profile (the depth profile of a set of intervals computed on the device in memory proportional to the intervals: metamaps_amd/csrc/mm_depth.hip,
mm_depth_core.hpp) through capi.py, exactly equal to the plain per-position restatement tests/depth_ref.py: the built cases of tests/depth_cases.py (63 / 64 /
65 and 255 / 256 / 257 intervals with distinct breakpoints, 70 000 identical intervals, abutting and nested intervals, a start on another's last + 1, contig
ends, a contig of one base, 1 000 contigs with three listed, every window shape, the median's rank around the zeros, no and eight thresholds), the contig of
2^29 - 1 bases against values written down by hand (one window, and 536 871 windows of 1 000), 200 seeded random worlds each run again with its intervals
permuted, the empty call, and every refusal with *out NULL and its message."""
import random

import numpy as np
import pytest

import depth_cases
import depth_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from metamaps_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def call(ctx, w):
    iv = w["iv"]
    got = ctx.depth_profile(w["lens"], [c for c, _, _ in iv], [a for _, a, _ in iv], [b for _, _, b in iv], window=w["W"], thresholds=w["T"])
    return dict(runs=list(zip(got["run_contig"].tolist(), got["run_start"].tolist(), got["run_end"].tolist(), got["run_depth"].tolist())), contig=got["contig"].tolist(),
                win_off=got["win_off"].tolist(), stats=got["stats"].tolist(), win_sum=got["win_sum"].tolist(), win_covered=got["win_covered"].tolist())


def expected(w):
    return depth_ref.profile(w["lens"], w["iv"], w["W"], w["T"])


@pytest.fixture(scope="module")
def built():
    worlds = depth_cases.built_worlds()
    return worlds, {name: expected(w) for name, w in worlds.items()}


def test_built_cases(ctx, built):
    worlds, want = built
    for name, w in worlds.items():
        assert call(ctx, w) == want[name], name
    assert want["abutting"]["runs"] == [(0, 0, 10, 1)] and want["coincide"]["runs"] == [(0, 0, 2, 1), (0, 2, 16, 2), (0, 16, 20, 1)]
    assert want["contig_end"]["runs"] == [(0, 5, 9, 1), (0, 9, 10, 2), (1, 0, 1, 2), (1, 1, 4, 1)] and want["three_of_1000"]["contig"] == [7, 500, 998]
    assert want["identical70000"]["stats"] == [[70_000, 16, 16 * 70_000, 70_000, 70_000, 16, 16, 16, 16, 0]]
    assert all(len(want[f"ladder{n}"]["runs"]) == 2 * n - 1 for n in (63, 64, 65, 255, 256, 257))


@pytest.mark.parametrize("window", [depth_cases.HUGE, 1000])
def test_the_contig_of_2_29_minus_1_bases(ctx, window):
    """sumDepth and a window's sum pass 2^32, positions 2^28; at W = 1000 there are 536 871 windows"""
    got, want = call(ctx, depth_cases.huge_world(window)), depth_cases.huge_expected(window)
    assert got["runs"] == want["runs"] and got["contig"] == want["contig"] and got["stats"] == want["stats"] and got["win_off"] == want["win_off"]
    assert np.array_equal(np.array(got["win_sum"]), np.array(want["win_sum"])) and np.array_equal(np.array(got["win_covered"]), np.array(want["win_covered"]))
    assert want["stats"][0][2] > 1 << 32 and want["win_off"][-1] == (1 if window == depth_cases.HUGE else 536_871)


@pytest.mark.parametrize("part", range(4))
def test_random_worlds_and_their_permutations(ctx, part):
    worlds = depth_cases.random_worlds()
    assert len(worlds) == 200
    rng = random.Random(part)
    for k in range(part, 200, 4):
        w = worlds[k]
        got = call(ctx, w)
        assert got == expected(w), k
        assert call(ctx, dict(w, iv=rng.sample(w["iv"], len(w["iv"])))) == got, k


def test_no_interval_gives_empty_sizes(ctx):
    got = call(ctx, depth_cases.world([10, 20], [], W=3, T=(1, 2)))
    assert got == dict(runs=[], contig=[], win_off=[0], stats=[], win_sum=[], win_covered=[]) and ctx.last_depth_handle not in (None, 0xDEAD)
    assert call(ctx, depth_cases.world([], [], W=3, T=()))["win_off"] == [0]


def test_refusals(ctx):
    from metamaps_amd import capi
    good, bad = depth_cases.refused_worlds()
    want = expected(good)
    assert call(ctx, good) == want

    def refused(w, *words):
        with pytest.raises(capi.MMError) as e:
            call(ctx, w)
        assert e.value.status == capi.MM_ERR_ARG and "mm_depth_profile" in str(e.value) and ctx.last_depth_handle is None, str(e.value)
        assert all(x in str(e.value) for x in words), (words, str(e.value))
        assert call(ctx, good) == want                              # a correct call follows on the same context
    for why, w in bad:
        refused(w, *({"length": ["length", "[1, 2^29)"], "window": ["window", str(w["W"])], "thresholds": ["thresholds"]}.get(why) or [why + " "]))
    # 5 * (2^29 - 1) windows of one base: the message says so and names the window
    refused(depth_cases.world([depth_cases.HUGE] * 5, [(c, 0, 0) for c in range(5)], W=1), "2^31 - 1 windows", "window 1 ")
    import ctypes as C
    one, h = np.ones(1, dtype=np.int64), C.c_void_p(0xDEAD)         # more than 2^29 contigs: refused on the count alone, before any length is read
    with pytest.raises(capi.MMError) as e:
        ctx.check(capi.lib().mm_depth_profile(ctx.h, (1 << 29) + 1, one.ctypes.data_as(C.c_void_p), 0, None, None, None, 1000, 0, None, C.byref(h)))
    assert e.value.status == capi.MM_ERR_ARG and "2^29 contigs" in str(e.value) and h.value is None
