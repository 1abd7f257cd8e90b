"""The worlds of the depth profile's tests (tests/test_depth_core.py on the host, tests/test_gpu_depth.py on the device): a world is a dict with lens (the
contigs' lengths), iv (the intervals (contig, first, last)), W (the window) and T (the thresholds).  The built cases sit on the edges of the definition and of
the kernels; the random worlds are seeded.  The contig of 2^29 - 1 bases has its expected values written down by hand: no per-position array can hold it."""
import random

DEFAULT_T = (1, 5, 10, 30)
HUGE = (1 << 29) - 1


def world(lens, iv, W=1000, T=DEFAULT_T):
    return dict(lens=list(lens), iv=[tuple(x) for x in iv], W=W, T=tuple(T))


def ladder(n):
    """n intervals on one contig with 2n distinct breakpoints: depth climbs to n and comes down again"""
    return world([4 * n + 3], [(0, 2 * i, 2 * n + 2 * i) for i in range(n)], W=7, T=(1, n // 2, n, n + 1))


def built_worlds():
    w = {}
    for n in (63, 64, 65, 255, 256, 257):                           # the wavefront and workgroup edges of the flat kernels and of the compaction
        w[f"ladder{n}"] = ladder(n)
    w["identical70000"] = world([30], [(0, 5, 20)] * 70_000, W=8, T=(1, 65_535, 65_536, 70_000, 70_001))   # depth passes 65 535 with two breakpoints
    w["abutting"] = world([12], [(0, 0, 4), (0, 5, 9)], W=5)                                          # one run [0, 10)
    w["coincide"] = world([20], [(0, 0, 19), (0, 2, 9), (0, 10, 15)], W=4, T=(1, 2, 3))                 # a start on another's last + 1: no new run
    w["nested"] = world([50], [(0, 5, 40), (0, 10, 30), (0, 15, 20), (0, 15, 25), (0, 15, 15), (0, 5, 5)], W=10, T=(1, 2, 3, 4, 5, 6))
    w["contig_end"] = world([10, 8], [(0, 5, 9), (1, 0, 3), (0, 9, 9), (1, 0, 0)], W=3, T=(1, 2))      # no run crosses
    w["length1"] = world([1, 1, 1], [(0, 0, 0), (2, 0, 0), (2, 0, 0)], W=1, T=(1, 2))
    w["three_of_1000"] = world([17 + c % 5 for c in range(1000)], [(7, 0, 16), (500, 3, 9), (500, 5, 12), (998, 1, 1)], W=6)
    w["last_contig"] = world([40, 40, 33], [(2, 0, 32), (2, 10, 20)], W=11)
    base = [(0, 3, 5), (0, 8, 8), (0, 10, 59), (0, 12, 14), (0, 70, 99)]                              # runs inside one window, a run over whole windows
    w["window1"] = world([100], base, W=1)
    w["window_over_len"] = world([100], base, W=101)
    w["window_is_len"] = world([100], base, W=100)
    w["len_kW"] = world([100], base, W=10)
    w["len_kW_1"] = world([101], base + [(0, 100, 100)], W=10)
    w["len_kW_1_empty_tail"] = world([101], base, W=10)
    w["window_huge"] = world([100], base, W=(1 << 63) - 1)
    # the median's rank (len - 1) // 2 against the zeros: len 10 has rank 4, len 11 rank 5
    w["median_in_zeros_even"] = world([10], [(0, 7, 8), (0, 8, 8)])
    w["median_last_zero_even"] = world([10], [(0, 5, 9), (0, 7, 9)])                                  # 5 zeros: rank 4 is the last of them
    w["median_first_covered_even"] = world([10], [(0, 4, 9), (0, 6, 9), (0, 6, 9)])                   # 4 zeros: rank 4 is the lowest covered depth
    w["median_last_zero_odd"] = world([11], [(0, 0, 4), (0, 0, 1)])                                   # 6 zeros: rank 5 is the last of them
    w["median_first_covered_odd"] = world([11], [(0, 0, 5), (0, 0, 1), (0, 3, 3)])                    # 5 zeros
    w["median_ties"] = world([11], [(0, 0, 10), (0, 0, 1), (0, 4, 5), (0, 8, 9), (0, 9, 9)])           # depth 2 in three runs, the median among them
    w["median_full_cover"] = world([9], [(0, 0, 8), (0, 0, 3), (0, 0, 3), (0, 6, 8)])
    w["no_thresholds"] = world([30], [(0, 1, 20), (0, 5, 9)], W=7, T=())
    w["eight_thresholds"] = world([30], [(0, 0, 29)] * 9 + [(0, k, 29 - k) for k in range(9)], W=7, T=(1, 2, 3, 5, 9, 10, 18, 19))   # the last above maxDepth
    return w


def random_worlds(n=200, seed=20261020):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        lens = [rng.choice((1, 2, 3, rng.randint(1, 300), rng.randint(200, 300))) for _ in range(rng.randint(1, 8))]
        iv = []
        for _ in range(rng.choice((1, 2, 5, rng.randint(1, 400)))):
            c = rng.randrange(len(lens))
            a = rng.randrange(lens[c])
            b = min(lens[c] - 1, a + rng.choice((0, 1, rng.randint(0, 20), rng.randint(0, 300))))
            iv.append((c, a, b))
        T = tuple(sorted(rng.sample(range(1, 40), rng.randint(0, 8))))
        out.append(world(lens, iv, W=rng.choice((1, 2, 7, 50, 64, 299, 300, 301, 1000)), T=T))
    return out


def huge_world(window=HUGE):
    """70 000 identical intervals over a whole contig of 2^29 - 1 bases (between two small contigs): sumDepth and a window's sum pass 2^32, positions 2^28"""
    return world([5, HUGE, 7], [(1, 0, HUGE - 1)] * 70_000, W=window, T=(1, 69_999, 70_000, 70_001))


def huge_expected(window=HUGE):
    """what huge_world gives, by hand"""
    n_win = (HUGE - 1) // window + 1
    last = HUGE - (n_win - 1) * window
    return dict(runs=[(1, 0, HUGE, 70_000)], contig=[1], win_off=[0, n_win], stats=[[70_000, HUGE, 70_000 * HUGE, 70_000, 70_000, HUGE, HUGE, HUGE, 0]],
                win_sum=[70_000 * window] * (n_win - 1) + [70_000 * last], win_covered=[window] * (n_win - 1) + [last])


def refused_worlds():
    """(why, world): every refusal of the call; `why` names a word its message holds"""
    good = world([10, 20], [(0, 0, 9), (1, 5, 7)], W=4, T=(1, 2))
    bad = [
        ("length", dict(good, lens=[10, 0])),
        ("length", dict(good, lens=[10, 1 << 29])),
        ("length", dict(good, lens=[-3, 20])),
        ("interval 1", dict(good, iv=[(0, 0, 9), (1, 5, 20), (1, 30, 40)])),                          # the lowest offending interval is named
        ("interval 0", dict(good, iv=[(0, 5, 4), (1, 5, 7)])),
        ("interval 1", dict(good, iv=[(0, 0, 9), (2, 0, 0)])),
        ("interval 1", dict(good, iv=[(0, 0, 9), (-1, 0, 0)])),
        ("interval 0", dict(good, iv=[(0, -1, 3)])),
        ("window", dict(good, W=0)),
        ("window", dict(good, W=-5)),
        ("thresholds", dict(good, T=(1, 2, 3, 4, 5, 6, 7, 8, 9))),
        ("thresholds", dict(good, T=(0, 2))),
        ("thresholds", dict(good, T=(2, 2))),
        ("thresholds", dict(good, T=(3, 2))),
    ]
    return good, bad
