"""The fused learners' replay sampling WITHOUT replacement (CN_SAMPLE_DISTINCT: cn_replay_row_distinct in csrc/crowdnav_learner_device.h, stated
in include/crowdnav.h next to cn_td3_batch_dev) as a CPU statement: exact integers, NumPy uint64 for the hashes and the rows, Python
ints for a, b and the key.  No kernel code and no libcrowdnav.

Row m of the handle's update number c, every integer an unsigned 64-bit one:
  n  = max(*replay_size_dev, 1)
  a  = the least integer with a*a >= n;   b = ceil(n / a)
  K  = mix64(seed ^ mix64(c ^ 0x9E3779B97F4A7C15))
  x  = m mod n
  repeat (at most 64 times):
      L = x / b;  R = x % b
      for i = 0..3:   i even: L = (L + mix64(mix64(K ^ (i+1)) ^ R)) % a
                      i odd : R = (R + mix64(mix64(K ^ (i+1)) ^ L)) % b
      x = L*b + R
  until x < n
  row = x            (x mod n if the 64th pass still left x >= n)
The sums are exact: h = mix64(..) is reduced first, (L + h % a) % a, so L + h never wraps at 2^64 (a wrapped sum would not be a
rotation of Z_a, and the rounds would not be invertible).  L, R < 2^32, so the reduced sums fit a uint64 with room to spare.

INDEX_VARIANTS are wrong statements the tests must be able to tell apart (sampling_f64.INDEX_VARIANTS' style)."""
import math

import numpy as np

from actor_f64 import MASK64, mix64

KEY_XOR = 0x9E3779B97F4A7C15
ROUNDS = 4
MAX_PASSES = 64

INDEX_VARIANTS = ("rounds3", "key_no_const", "ab_swapped", "m_raw", "capacity")

# ---- the GPU test's plan (tests/test_gpu_replay_distinct.py), here so that the CPU tests can show it tells the variants apart ----
LIVE_SIZES = (1, 2, 3, 37, 63, 64, 65, 4096, 5003, 65536, 1_000_000, (1 << 24) + 1)
DEGENERATE_SIZES = (0, -1)                      # *size_dev values taken as 1
BATCHES = (1, 129, 4096)
SEEDS = (0, MASK64, 0x6A09E667F3BCC908)
COUNTERS = (0, 1, 1 << 32, MASK64)
CAPACITY = (1 << 24) + 4099                     # what the "capacity" variant divides by instead of the live size


def live(size):
    """max(size, 1): an int64 on the device; 0 and negatives are taken as 1."""
    return max(int(size), 1)


def domain(n):
    """(a, b): a = ceil(sqrt(n)), b = ceil(n / a), in Python ints."""
    n = int(n)
    a = math.isqrt(n - 1) + 1
    return a, -(-n // a)


def _mix_int(z):
    return int(mix64(np.array([int(z) & MASK64], dtype=np.uint64))[0])


def key(seed, counter, variant=None):
    c = int(counter) & MASK64
    return _mix_int((int(seed) & MASK64) ^ _mix_int(c if variant == "key_no_const" else c ^ KEY_XOR))


def rows(seed, counter, B, size, variant=None, capacity=None, ms=None, passes=None):
    """Ring rows (int64) of batch rows 0 .. B-1 (or of the listed `ms`) of update `counter`.  variant: one of INDEX_VARIANTS -- three
    rounds, the key without its constant, a and b exchanged, m instead of m mod n, the ring's capacity (`capacity`) instead of
    its live size.  passes: a list that receives the largest number of passes any row took."""
    n = live(capacity if variant == "capacity" else size)
    a, b = domain(n)
    if variant == "ab_swapped":
        a, b = b, a
    K = key(seed, counter, variant)
    ks = [np.uint64(_mix_int(K ^ (i + 1))) for i in range(ROUNDS)]
    m = (np.arange(B, dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)).astype(np.uint64)
    un, ua, ub = np.uint64(n), np.uint64(a), np.uint64(b)
    x = m.copy() if variant == "m_raw" else m % un
    out = np.zeros(x.shape, dtype=np.uint64)
    todo = np.ones(x.shape, dtype=bool)
    worst = 0
    for p in range(MAX_PASSES):
        if not todo.any():
            break
        worst = p + 1
        xt = x[todo]
        L, R = xt // ub, xt % ub
        for i in range(3 if variant == "rounds3" else ROUNDS):
            if i % 2 == 0:
                L = (L + mix64(ks[i] ^ R) % ua) % ua
            else:
                R = (R + mix64(ks[i] ^ L) % ub) % ub
        xt = L * ub + R
        x[todo] = xt
        done = todo.copy()
        done[todo] = xt < un
        out[done] = x[done]
        todo &= ~done
    out[todo] = x[todo] % un
    if passes is not None:
        passes.append(worst)
    return out.astype(np.int64)


def chi2_rows(draws, n):
    """Pearson's chi-square of how often each of the n ring rows occurs in `draws` (any shape) against the uniform expectation."""
    cnt = np.bincount(np.asarray(draws).reshape(-1), minlength=n).astype(np.float64)
    e = cnt.sum() / n
    return float(((cnt - e) ** 2 / e).sum())


def chi2_pairs(first, second, n):
    """Pearson's chi-square of the ordered pair (first, second), first != second, over the n (n - 1) possible pairs."""
    first, second = np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)
    assert (first != second).all()
    cnt = np.bincount(first * n + second, minlength=n * n).astype(np.float64).reshape(n, n)
    off = ~np.eye(n, dtype=bool)
    e = len(first) / (n * (n - 1))
    return float(((cnt[off] - e) ** 2 / e).sum())
