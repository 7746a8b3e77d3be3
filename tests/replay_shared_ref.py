"""A population's shared replay source (CN_REPLAY_SHARED: cn_replay_row_shared in csrc/crowdnav_learner_device.h, stated in
include/crowdnav.h next to cn_td3_pop_update) as a CPU statement: NumPy for the draw over the union, Python ints for the sizes and
their prefix sums.  No kernel code and no libcrowdnav.

Batch row m of member p at its update number c, every integer an unsigned 64-bit one:
  n_q   = max(*replay_size_dev of member q, 0)          q = 0 .. P-1
  pre_q = n_0 + ... + n_{q-1}                            (pre_0 = 0)
  N     = max(pre_P, 1)
  x     = the one-ring row for (seed_p, c, m) with live size N: sampling_f64.indices (CN_SAMPLE_WITH_REPLACEMENT) or
          replay_distinct_ref.rows (CN_SAMPLE_DISTINCT)
  q*    = the least q with x < pre_{q+1};  none (every ring empty): q* = p
  row   = x - pre_{q*}                                   (0 when every ring is empty)

PAIR_VARIANTS are wrong statements the tests must be able to tell apart (sampling_f64.INDEX_VARIANTS' style)."""
import numpy as np

import replay_distinct_ref
import sampling_f64
from actor_f64 import MASK64

WITH_REPLACEMENT, DISTINCT = 0, 1
PAIR_VARIANTS = ("inclusive_prefix", "own_size", "capacity", "ring_then_row", "seed0")


def live_sizes(sizes):
    """n_q: negatives count as empty rings."""
    return [max(int(s), 0) for s in sizes]


def prefixes(sizes):
    """[pre_0 .. pre_P] in Python ints."""
    pre = [0]
    for n in live_sizes(sizes):
        pre.append(pre[-1] + n)
    return pre


def union_rows(seed, counter, B, N, mode):
    """x of batch rows 0 .. B-1 over a union of N >= 1 live rows (int64)."""
    if mode == DISTINCT:
        return replay_distinct_ref.rows(seed, counter, B, N)
    return sampling_f64.indices(seed, counter, B, N)


def pairs(seeds, counter, B, sizes, member, mode, variant=None, capacities=None):
    """{q*, row} [B, 2] (int64) of member `member`'s batch rows 0 .. B-1 at its update number `counter`.  seeds: the members' seeds
    (or one int, for all); sizes: the members' *replay_size_dev.  variant: one of PAIR_VARIANTS -- the seam taken with <= (an
    inclusive prefix), the member's own size instead of N, the rings' `capacities` instead of their live sizes, a ring drawn
    uniformly and then a row of it, member 0's seed for every member."""
    P = len(sizes)
    seeds = [int(seeds)] * P if np.isscalar(seeds) or isinstance(seeds, int) else [int(s) for s in seeds]
    seed = (seeds[0] if variant == "seed0" else seeds[member]) & MASK64
    n = live_sizes(capacities if variant == "capacity" else sizes)
    pre = prefixes(n)
    out = np.zeros((B, 2), dtype=np.int64)
    if variant == "ring_then_row":
        out[:, 0] = q = union_rows(seed, counter, B, P, mode)
        for ring in set(q.tolist()):
            out[q == ring, 1] = union_rows(seed, counter, B, max(n[ring], 1), mode)[q == ring]
        return out
    N = max(n[member] if variant == "own_size" else pre[P], 1)
    x = union_rows(seed, counter, B, N, mode)
    if pre[P] == 0:
        out[:, 0] = member
        return out
    ends = np.array(pre[1:], dtype=np.int64)
    q = np.searchsorted(ends, x, side="left" if variant == "inclusive_prefix" else "right")      # the least q with x < (<=) pre_{q+1}
    q = np.minimum(q, P - 1)                           # (own_size: x < n_member <= pre_P always; the clamp never acts in the statement)
    out[:, 0] = q
    out[:, 1] = x - np.array(pre, dtype=np.int64)[q]
    return out


def chi2_uniform(counts):
    """Pearson's chi-square of `counts` against the uniform expectation."""
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


# ---- the GPU tests' plan (tests/test_gpu_replay_shared.py), here so that the CPU tests can show it tells the variants apart --------
BIG = ((1 << 24) + 1, 1, 0, 1_000_000)
SIZE_TUPLES = ((1,), (0, 0, 0), (0, 5, 0), (1, 1, 1), (37, 0, 64), (64, 65, 63), tuple(i % 5 for i in range(64)), BIG, (5, -3, 2))
SMALL = 1000                                        # tuples whose union is smaller also run B = N and B = N + 1
SEEDS = (0, MASK64)
COUNTERS = (0, 1 << 32, MASK64)
MODES = (WITH_REPLACEMENT, DISTINCT)
# BIG's seams lie 2^24 rows into a union of 17.7 million: a draw of 129 rows reaches them only by search.  (seed, counter, mode, B)
# whose rows include x = 2^24, 2^24 + 1 and 2^24 + 2 -- both sides of the seams pre_1 and pre_2 = pre_3 (found by scanning counters
# with this file; test_plan_reaches_both_sides_of_every_seam checks them).
SEAM_CASES = ((0, 372669, WITH_REPLACEMENT, 129), (0, 184258, WITH_REPLACEMENT, 129), (0, 126391, WITH_REPLACEMENT, 129))


def capacities_of(sizes):
    """What the "capacity" variant takes for the live sizes: rings a little larger than what they hold."""
    return [max(int(s), 0) + 3 for s in sizes]


def sample_plan():
    """[(sizes, B, member, seed, counter, mode)] of the sampling test."""
    plan = []
    for sizes in SIZE_TUPLES:
        P, N = len(sizes), max(prefixes(sizes)[-1], 1)
        batches = (1, 129) + ((N, N + 1) if N < SMALL else ())
        for B in dict.fromkeys(batches):
            for member in dict.fromkeys((0, P - 1)):
                for seed in SEEDS:
                    for counter in COUNTERS:
                        for mode in MODES:
                            plan.append((sizes, B, member, seed, counter, mode))
    for seed, counter, mode, B in SEAM_CASES:
        plan.append((BIG, B, 0, seed, counter, mode))
    return plan


def seams(sizes):
    """The union indices on either side of every seam between two rings that lies inside the union: pre_q - 1 and pre_q."""
    pre = prefixes(sizes)
    return sorted({x for q in range(1, len(sizes)) if 0 < pre[q] < pre[-1] for x in (pre[q] - 1, pre[q])})


# the update test's members: live sizes per member, and the seeds tests/test_gpu_td3_population.Member gives to key = 0, 1, 2
UPDATE_SIZES = ((300, 0, 7), (300, 7), (64, 64, 64), (64, 64))
UPDATE_SEEDS = tuple((0x9E3779B97F4A7C15 * (k + 1)) & MASK64 for k in range(3))
UPDATE_BATCHES = (40, 33, 128)
