"""CPU checks of tests/replay_shared_ref.py, the statement the GPU tests hold CN_REPLAY_SHARED to: its draw is uniform over the
union's live rows, distinct where the mode says so, degenerate cases are what the header says, and the wrong variants are told
apart on the GPU tests' own plans."""
import numpy as np
import pytest

import replay_distinct_ref
import replay_shared_ref as S
import sampling_f64
from actor_f64 import MASK64

# The 0.999 quantile of chi-square at 101 degrees of freedom (Wilson-Hilferty: 101 (1 - 2/909 + 3.0902 sqrt(2/909))^3 = 150.7; tables: 150.67)
CHI2_999_DF101 = 150.67


def _union_index(pr, sizes):
    pre = np.array(S.prefixes(sizes), dtype=np.int64)
    return pre[pr[:, 0]] + pr[:, 1]


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("seed", (3, 0xBB67AE8584CAA73B))
def test_the_draw_is_uniform_over_the_unions_live_rows(seed, mode):
    """2 * 10^5 indices over sizes (37, 0, 64, 1): 102 live rows, 101 degrees of freedom.  A condition, not a measurement.  Figures
    (seed 3 / 0xBB67...): with replacement 112.9 / 102.6; distinct rows, 16 a batch, 80.6 / 90.1."""
    sizes = (37, 0, 64, 1)
    B = 16
    n = sum(S.live_sizes(sizes))
    draws = np.concatenate([S.pairs(seed, c, B, sizes, c % 4, mode) for c in range(200_000 // B)])
    assert len(draws) == 200_000
    assert (draws[:, 0] != 1).all()                                   # the empty ring is never drawn
    for q, nq in enumerate(sizes):
        assert (draws[draws[:, 0] == q, 1] < max(nq, 1)).all()
    chi2 = S.chi2_uniform(np.bincount(_union_index(draws, sizes), minlength=n))
    print("\nseed %#x mode %d: chi2 %.1f (< %.2f)" % (seed, mode, chi2, CHI2_999_DF101))
    assert chi2 < CHI2_999_DF101


def test_distinct_pairs_below_the_union_and_a_permutation_at_it():
    for sizes in ((37, 0, 64, 1), (1, 1, 1), (0, 5, 0), (64, 65, 63), tuple(i % 5 for i in range(64))):
        n = sum(S.live_sizes(sizes))
        for c in (0, 1 << 32, MASK64):
            for member in (0, len(sizes) - 1):
                full = S.pairs(9, c, n, sizes, member, S.DISTINCT)
                assert np.array_equal(np.sort(_union_index(full, sizes)), np.arange(n)), (sizes, c)
                for B in {1, max(n // 2, 1), n - 1} - {0}:
                    part = S.pairs(9, c, B, sizes, member, S.DISTINCT)
                    assert len({tuple(r) for r in part.tolist()}) == B, (sizes, c, B)
                    assert np.array_equal(part, full[:B])


def test_all_rings_empty_gives_the_member_and_row_zero():
    for sizes in ((0,), (0, 0, 0), (0, -4, 0), (-1,) * 64):
        for member in range(len(sizes)):
            for mode in S.MODES:
                got = S.pairs(5, 7, 33, sizes, member, mode)
                assert (got[:, 0] == member).all() and not got[:, 1].any(), (sizes, member, mode)


def test_one_member_is_the_one_ring_statement():
    for size in (1, 2, 37, 64, 65, 5003, (1 << 24) + 1, 0, -1):
        for seed in S.SEEDS:
            for c in S.COUNTERS:
                got = S.pairs(seed, c, 129, (size,), 0, S.WITH_REPLACEMENT)
                assert not got[:, 0].any() and np.array_equal(got[:, 1], sampling_f64.indices(seed, c, 129, size))
                got = S.pairs(seed, c, 129, (size,), 0, S.DISTINCT)
                assert not got[:, 0].any() and np.array_equal(got[:, 1], replay_distinct_ref.rows(seed, c, 129, size))


def test_negative_sizes_are_empty_rings():
    assert np.array_equal(S.pairs(1, 2, 50, (5, -3, 2), 1, 0), S.pairs(1, 2, 50, (5, 0, 2), 1, 0))
    assert S.prefixes((5, -3, 2)) == [0, 5, 5, 7]


def test_plan_reaches_both_sides_of_every_seam():
    """For every size tuple of the sampling plan, every union index next to a seam (pre_q - 1 and pre_q) is drawn by some case."""
    seen = {}
    for sizes, B, member, seed, c, mode in S.sample_plan():
        want = S.seams(sizes)
        if want:
            x = _union_index(S.pairs(seed, c, B, sizes, member, mode), sizes)
            seen.setdefault(sizes, set()).update(set(want) & set(x.tolist()))
    for sizes in S.SIZE_TUPLES:
        assert seen.get(sizes, set()) == set(S.seams(sizes)), (sizes[:8], sorted(set(S.seams(sizes)) - seen.get(sizes, set())))
    assert S.seams(S.BIG) == [1 << 24, (1 << 24) + 1, (1 << 24) + 2] and S.seams((0, 5, 0)) == [] and S.seams((1, 1, 1)) == [0, 1, 2]


@pytest.mark.parametrize("variant", S.PAIR_VARIANTS)
def test_wrong_variants_differ_on_the_gpu_tests_plans(variant):
    """The sampling plan passes one seed, so "seed0" can only show in the update test's plan (members with seeds of their own); the
    other four must show in both."""
    differs = total = 0
    if variant != "seed0":
        for sizes, B, member, seed, c, mode in S.sample_plan():
            total += 1
            differs += not np.array_equal(S.pairs(seed, c, B, sizes, member, mode),
                                          S.pairs(seed, c, B, sizes, member, mode, variant=variant, capacities=S.capacities_of(sizes)))
        print("\n%s: differs on %d of %d sampling cases" % (variant, differs, total))
        assert differs > 0
    hit = 0
    for sizes in S.UPDATE_SIZES:
        for B in S.UPDATE_BATCHES:
            for mode in S.MODES:
                for c in range(4):
                    for member in range(len(sizes)):
                        hit += not np.array_equal(S.pairs(S.UPDATE_SEEDS, c, B, sizes, member, mode),
                                                  S.pairs(S.UPDATE_SEEDS, c, B, sizes, member, mode, variant=variant,
                                                          capacities=S.capacities_of(sizes)))
    print("%s: differs on %d update cases" % (variant, hit))
    assert hit > 0
