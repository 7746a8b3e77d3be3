"""NumPy restatement of cn_pop_record's statement (include/crowdnav.h) for one member, and the makers of the cases that
tests/test_pop_record_layout.py (CPU, against the PyTorch formulations) and tests/test_gpu_pop_record.py (against the per-member
kernels) share.  A member is a dict of arrays; record() changes it in place exactly as the header says the call does."""
import numpy as np

SENTINEL = -777.0          # padding rows behind every buffer: they must survive a call
PAD = 3


def kernel_order_sum(x):
    """The float64 sum of cn_episode_log_kernel: thread t of 1024 adds its rows i = t (mod 1024) in ascending order, the 64 lanes of a
    wavefront are combined by the xor-shuffle butterfly (32, 16, ..., 1; lane 0's value), the 16 wave totals are added in order."""
    x = np.asarray(x, dtype=np.float64)
    part = np.zeros(1024, dtype=np.float64)
    for base in range(0, len(x), 1024):
        seg = x[base:base + 1024]
        part[:len(seg)] = part[:len(seg)] + seg
    lanes = part.reshape(16, 64).copy()
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ m]
    v = np.float64(0.0)
    for w in range(16):
        v = v + lanes[w, 0]
    return v


def record(m, launch):
    """cn_pop_record for one member, in place.  m: ring arrays s, s2 [>= cap, D], a [>= cap, 2], r, d [>= cap], cap, pos, size; log
    rows [>= max_rows, 8], max_rows, n_log, tot [5] float64; prev, obs [>= n, D], action [>= n, 2], reward, done, resetting [>= n];
    counters [>= n, 14] int32, last_return [>= n]; n."""
    n, cap = m["n"], m["cap"]
    if n == 0:
        return m
    keep = m["resetting"][:n] == 0
    rank = np.cumsum(keep)
    slots = (m["pos"] + rank - 1) % cap
    for i in np.nonzero(keep)[0]:
        sl = slots[i]
        m["s"][sl] = m["prev"][i]; m["s2"][sl] = m["obs"][i]; m["a"][sl] = m["action"][i]
        m["r"][sl] = m["reward"][i]; m["d"][sl] = 1.0 if m["done"][i] else 0.0
    kept = int(keep.sum())
    m["pos"] = (m["pos"] + kept) % cap
    m["size"] = min(m["size"] + kept, cap)
    done = m["done"][:n] != 0
    cf = m["counters"][:n].astype(np.float32)
    ret = m["last_return"][:n].astype(np.float32)
    at = m["n_log"] + np.cumsum(done) - 1
    for i in np.nonzero(done)[0]:
        if at[i] < m["max_rows"]:
            m["rows"][at[i]] = (cf[i, 4], cf[i, 5], ret[i], cf[i, 13], cf[i, 10], cf[i, 11], cf[i, 12], np.float32(launch))
    m["n_log"] += int(done.sum())
    df = done.astype(np.float64)
    m["tot"] = m["tot"] + np.array([kernel_order_sum(df), kernel_order_sum(cf[:, 4].astype(np.float64) * df),
                                    kernel_order_sum(np.where(done, ret.astype(np.float64), 0.0)),
                                    kernel_order_sum(cf[:, 13].astype(np.float64) * df), kernel_order_sum(keep.astype(np.float64))])
    m["resetting"][:n] = done
    m["prev"][:n] = m["obs"][:n]
    return m


PATTERNS = ("all", "none", "alternating", "last", "row1024")


def pattern(name, n):
    """A byte pattern over n rows: all, none, alternating (odd rows), only the last row, only row 1024 (none below 1025 rows)."""
    x = np.zeros(n, dtype=np.uint8)
    if name == "all":
        x[:] = 1
    elif name == "alternating":
        x[1::2] = 1
    elif name == "last" and n:
        x[-1] = 1
    elif name == "row1024" and n > 1024:
        x[1024] = 1
    return x


def mixed_returns(rng, n, lo=-3, hi=4):
    """Returns of magnitude 10^lo ... 10^hi (1e-3 ... 1e4), both signs.  Widened float32 values this close together still add up
    almost exactly in float64; lo, hi = -12, 12 ("wide") is the spread at which the order of the float64 sum shows in its bits."""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


def make_member(rng, n, D, cap=None, pos=0, size=0, max_rows=None, n_log=0, done="alternating", resetting="none", returns="mixed"):
    """One member with chosen patterns; every buffer carries PAD sentinel rows behind its last row.  cap / max_rows default to room
    for everything."""
    cap = max(n, 1) + 5 if cap is None else cap
    max_rows = n + 7 if max_rows is None else max_rows
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)

    def padded(a, rows):
        out = np.full((rows + PAD,) + a.shape[1:], SENTINEL, dtype=a.dtype)
        out[:rows] = a
        return out
    ret = {"mixed": lambda: mixed_returns(rng, n), "wide": lambda: mixed_returns(rng, n, -12, 12),
           "exact": lambda: (rng.integers(-8000, 8000, n) / 8.0).astype(np.float32)}[returns]()
    cnt = rng.integers(0, 300, (n, 14)).astype(np.int32)
    cnt[:, 4] = rng.integers(0, 2, n); cnt[:, 5] = 1 - cnt[:, 4]
    m = dict(n=n, D=D, cap=cap, pos=pos, size=size, max_rows=max_rows, n_log=n_log,
             s=padded(f(cap, D), cap), s2=padded(f(cap, D), cap), a=padded(f(cap, 2), cap), r=padded(f(cap), cap), d=padded(f(cap), cap),
             rows=padded(f(max_rows, 8), max_rows), tot=rng.standard_normal(5) * 100.0,
             prev=padded(f(n, D), n), obs=padded(f(n, D), n), action=padded(f(n, 2), n), reward=padded(f(n), n),
             done=np.concatenate([pattern(done, n), np.full(PAD, 1, np.uint8)]),
             resetting=np.concatenate([pattern(resetting, n), np.full(PAD, 9, np.uint8)]),
             counters=padded(cnt, n), last_return=padded(ret, n))
    return m


def copy_member(m):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}


ARRAYS = ("s", "s2", "a", "r", "d", "rows", "tot", "prev", "obs", "action", "reward", "done", "resetting", "counters", "last_return")
SCALARS = ("pos", "size", "n_log")


def assert_members_equal(got, want, what=""):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, np.argwhere(a != b)[:4].tolist())
