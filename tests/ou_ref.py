"""cn_ddpg_act's noise (csrc/crowdnav_ddpg.hip; stated at cn_ddpg_act_io in include/crowdnav.h) restated in NumPy and Python ints:
the device draw U(seed, counter, row, component) and the Ornstein-Uhlenbeck update.  tests/test_ou_ref_helpers.py holds this file to
the reference's recorded process; tests/test_gpu_ddpg_act.py holds the kernel to this file."""
import numpy as np

M64 = (1 << 64) - 1
OU_TAG = 0x4F55


def mix64(z):
    """cn_mix64 (csrc/crowdnav_device.h) on Python ints, 64-bit wrap-around."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, counter, row, o):
    """U = (mix64(mix64(seed ^ mix64(counter ^ 0x4F55)) ^ (2 row + o)) >> 11) * 2^-53: 53 bits, as random.random()."""
    h = mix64(mix64((seed & M64) ^ mix64((counter & M64) ^ OU_TAG)) ^ ((2 * row + o) & M64))
    return (h >> 11) * 2.0 ** -53           # an integer below 2^53 times a power of two: exact


def draws(seed, counter, n):
    """[n, 2] float64: the uniforms of one call."""
    return np.array([[draw(seed, counter, e, o) for o in (0, 1)] for e in range(n)], dtype=np.float64)


def update(x, u, mu=0.0, theta=0.15, sigma=0.2, reset=None):
    """x1 = x0 + (theta (mu - x0) + sigma U), x0 = mu on the rows where `reset` is set: four float64 operations, each rounded on its
    own (NumPy does not contract).  x, u: [n, 2] float64; reset: [n] or None."""
    x = np.array(x, dtype=np.float64)
    if reset is not None:
        x[np.asarray(reset).astype(bool)] = mu
    drift = np.float64(theta) * (np.float64(mu) - x)
    kick = np.float64(sigma) * np.asarray(u, dtype=np.float64)
    return x + (drift + kick)


def action(pi, x1, max_v=0.22, max_w=2.0):
    """clip((float)((double)pi + x1)): numpy's float32 `action += noise` with a float64 noise, then ddpg.py:191-192."""
    a = (np.asarray(pi, dtype=np.float32).astype(np.float64) + x1).astype(np.float32)
    lo, hi = np.array([0.0, -max_w], dtype=np.float32), np.array([max_v, max_w], dtype=np.float32)
    return np.minimum(np.maximum(a, lo), hi)
