"""CPU checks of tests/replay_distinct_ref.py, the statement the GPU tests hold CN_SAMPLE_DISTINCT to: it is a permutation, its domain
wastes at most a quarter, its cycle walk is short, the wrong variants are told apart on the GPU test's own plan, and its draws pass
the same chi-square conditions as random.sample."""
import random

import numpy as np
import pytest

import replay_distinct_ref as S
import sampling_f64

PERM_SIZES = tuple(range(1, 301)) + (4096, 5003)
PERM_COUNTERS = (0, 1, (1 << 64) - 1)
PASSES = []


def test_rows_are_a_permutation_of_the_ring():
    for n in PERM_SIZES:
        want = np.arange(n)
        for c in PERM_COUNTERS:
            got = S.rows(3, c, n, n, passes=PASSES)
            assert got.min() >= 0 and got.max() < n and np.array_equal(np.sort(got), want), (n, c)
    # distinct below a full ring, too: a prefix of a permutation
    for n, B in ((65, 64), (5003, 128), ((1 << 24) + 1, 4096)):
        got = S.rows(S.SEEDS[2], 7, B, n, passes=PASSES)
        assert len(set(got.tolist())) == B and got.max() < n


def test_domain_covers_the_ring_and_wastes_at_most_a_quarter():
    n = np.arange(1, 100_000, dtype=np.int64)
    a = np.array([S.domain(int(v))[0] for v in n], dtype=np.int64)
    b = -(-n // a)
    assert np.array_equal(b, np.array([S.domain(int(v))[1] for v in n]))
    assert (a * a >= n).all() and ((a - 1) * (a - 1) < n).all()
    assert (a * b >= n).all() and (4 * (a * b - n) <= a * b).all()
    worst = ((a * b - n) / (a * b)).max()
    print("\nworst share of the a*b domain outside [0, n) for n < 100000: %.4f" % worst)
    assert worst <= 0.25
    for big in ((1 << 24) + 1, (1 << 31) + 11, (1 << 62) + 3, (1 << 63) - 1):
        a_, b_ = S.domain(big)
        assert a_ * a_ >= big > (a_ - 1) ** 2 and a_ * b_ >= big and 4 * (a_ * b_ - big) <= a_ * b_ and a_ * b_ < 1 << 64


def test_passes_stay_far_below_the_cap():
    if not PASSES:
        test_rows_are_a_permutation_of_the_ring()
    for n in S.LIVE_SIZES:
        for seed in S.SEEDS:
            S.rows(seed, 1 << 32, min(n, 4096), n, passes=PASSES)
    print("\nlargest number of passes over %d calls: %d (cap %d)" % (len(PASSES), max(PASSES), S.MAX_PASSES))
    assert max(PASSES) < S.MAX_PASSES


def test_more_rows_than_the_ring_holds():
    """B > n: x = m mod n, so every ring row comes up floor(B / n) or ceil(B / n) times."""
    for n, B in ((37, 128), (1, 5), (3, 129), (64, 129)):
        cnt = np.bincount(S.rows(11, 2, B, n), minlength=n)
        assert set(cnt.tolist()) <= {B // n, -(-B // n)}, (n, B)


def test_degenerate_sizes_are_one_row():
    for size in S.DEGENERATE_SIZES + (-(1 << 63),):
        assert not S.rows(5, 9, 129, size).any()


def test_scalar_python_restatement_agrees():
    """The statement once more with Python ints only (no NumPy wrap-around anywhere), row by row."""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def row(seed, c, m, n):
        a, b = S.domain(n)
        K = mix(seed ^ mix(c ^ 0x9E3779B97F4A7C15))
        x = m % n
        for _ in range(64):
            L, R = divmod(x, b)
            for i in range(4):
                if i % 2 == 0:
                    L = (L + mix(mix(K ^ (i + 1)) ^ R)) % a
                else:
                    R = (R + mix(mix(K ^ (i + 1)) ^ L)) % b
            x = L * b + R
            if x < n:
                return x
        return x % n

    for seed in S.SEEDS:
        for c in S.COUNTERS:
            for n in (1, 2, 37, 65, 5003, (1 << 24) + 1):
                ms = [0, 1, 63, 128, 4095]
                assert S.rows(seed, c, 0, n, ms=ms).tolist() == [row(seed, c, m, n) for m in ms], (seed, c, n)


@pytest.mark.parametrize("variant", S.INDEX_VARIANTS)
def test_wrong_variants_differ_on_the_gpu_tests_plan(variant):
    differs = total = 0
    for n in S.LIVE_SIZES:
        for B in S.BATCHES:
            for seed in S.SEEDS:
                for c in S.COUNTERS:
                    total += 1
                    differs += not np.array_equal(S.rows(seed, c, B, n), S.rows(seed, c, B, n, variant=variant, capacity=S.CAPACITY))
    print("\n%s: differs on %d of %d cases" % (variant, differs, total))
    assert differs > 0
    # and on the learners' cases (three counters each): n = B = 64 is a perfect square (a == b), the other two are not
    cases = [(64, 64), (65, 64), (5003, 128), (37, 128)]
    hit = [not np.array_equal(S.rows(9, c, B, n), S.rows(9, c, B, n, variant=variant, capacity=8192)) for n, B in cases for c in range(3)]
    assert any(hit), variant


def test_mode_one_is_not_the_draw_with_replacement():
    assert not np.array_equal(S.rows(3, 0, 64, 64), sampling_f64.indices(3, 0, 64, 64))
    assert len(set(sampling_f64.indices(3, 0, 64, 64).tolist())) < 64          # what the default mode gives on a full small ring


def test_draws_pass_the_chi_square_conditions_random_sample_passes():
    """Seed 3, counters 0..4095, n = 64, B = 16.  Conditions, not measurements: the 99.9 % quantiles of chi-square at 63 degrees of
    freedom (103.4: how often each ring row is drawn) and at 4031 (4308: the ordered pair (row 0's index, row 1's index) over its
    4032 possible values).  random.Random(3).sample is held to the same two bounds beside it, which shows the yardstick passes.
    Figures: the statement 47.3 and 4064.5, random.sample 55.9 and 3936.5.  (mix64 is the tree's cn_mix64, which adds splitmix64's
    increment before the finaliser; the same statement on the bare finaliser gives 58.1 and 4021.2.)"""
    n, B, C = 64, 16, 4096
    ours = np.stack([S.rows(3, c, B, n) for c in range(C)])
    rng = random.Random(3)
    theirs = np.array([rng.sample(range(n), B) for _ in range(C)])
    fig = {}
    for name, d in (("statement", ours), ("random.sample", theirs)):
        assert all(len(set(r)) == B for r in d.tolist())
        fig[name] = (S.chi2_rows(d, n), S.chi2_pairs(d[:, 0], d[:, 1], n))
        print("\n%-13s chi2 rows %.1f (< 103.4)   chi2 ordered pairs %.1f (< 4308)" % ((name,) + fig[name]))
    for name, (rows_, pairs) in fig.items():
        assert rows_ < 103.4, (name, rows_)
        assert pairs < 4308, (name, pairs)
