"""NumPy restatement of cn_nstep_record's statement (include/crowdnav.h) for one member, in float32 with every product and every
sum rounded on its own, and the makers of the cases that tests/test_nstep_ref_helpers.py (CPU) and tests/test_gpu_nstep_record.py
share.  A member is tests/pop_record_ref.py's dict with the window W, the one-step gamma and the pending store (ps [n, W, D],
pa [n, W, 2], pret [n, W], count [n], clock [n]); record() changes it in place exactly as the header says the call does."""
import numpy as np

import pop_record_ref as R

PENDING = ("ps", "pa", "pret", "count", "clock")
NSTEP_MAX = 16


def discount(gamma, k):
    """cn_nstep_discount: acc = 1.0 in float64, k multiplications by (double)(float)gamma, one cast to float.  No pow."""
    g, acc = float(np.float32(gamma)), 1.0
    for _ in range(k):
        acc *= g
    return np.float32(acc)


def add_pending(m, W, gamma):
    """Member m (pop_record_ref.make_member) with an empty pending store for window W."""
    n, D = m["n"], m["D"]
    m.update(W=W, gamma=np.float32(gamma), ps=np.zeros((n, W, D), np.float32), pa=np.zeros((n, W, 2), np.float32),
             pret=np.zeros((n, W), np.float32), count=np.zeros(n, np.int32), clock=np.zeros(n, np.int32))
    return m


def record(m, launch):
    """cn_nstep_record for one member, in place -> the ring rows emitted, as a list of (env, s, a, ret, s2, d)."""
    n, cap, W = m["n"], m["cap"], m["W"]
    out = []
    if n == 0:
        return out
    w = [discount(m["gamma"], k) for k in range(W)]
    keep = m["resetting"][:n] == 0
    for e in np.nonzero(keep)[0]:
        c0, k0 = int(m["count"][e]), int(m["clock"][e])
        r = np.float32(m["reward"][e])
        for k in range(1, c0 + 1):                             # the entry of age k: one float32 product, one float32 sum
            s = (k0 - k) % W
            m["pret"][e, s] = np.float32(m["pret"][e, s] + np.float32(w[k] * r))
        old = [(k0 - c0 + q) % W for q in range(c0)]           # the pending entries' slots, oldest first
        rows = [(m["ps"][e, s].copy(), m["pa"][e, s].copy(), m["pret"][e, s]) for s in old]
        new = (m["prev"][e].copy(), m["action"][e].copy(), m["reward"][e])     # the return is assigned: -0.0f survives
        fin = m["done"][e] != 0
        if fin:
            emit = rows + [new]
            m["count"][e] = m["clock"][e] = 0
        else:
            emit = (rows + [new])[:1] if c0 + 1 == W else []
            if W > 1:                                          # the new entry stays pending, in the one free slot
                s = k0 % W
                m["ps"][e, s], m["pa"][e, s], m["pret"][e, s] = new
            m["count"][e], m["clock"][e] = c0 + 1 - len(emit), k0 + 1
        out += [(int(e), s_, a_, ret, m["obs"][e].copy(), np.float32(1.0 if fin else 0.0)) for s_, a_, ret in emit]
    for q, (_, s_, a_, ret, s2, d) in enumerate(out):
        sl = (m["pos"] + q) % cap
        m["s"][sl], m["a"][sl], m["r"][sl], m["s2"][sl], m["d"][sl] = s_, a_, ret, s2, d
    # the episode log, tot[4] = the kept rows, resetting <- done and prev <- obs are cn_pop_record's: its restatement, run on copies of
    # the ring (its one-step rows are not wanted); rows, resetting and prev are shared arrays, the two scalars come back by value
    plain = dict(m, **{k: m[k].copy() for k in ("s", "s2", "a", "r", "d")})
    R.record(plain, launch)
    m["tot"], m["n_log"] = plain["tot"], plain["n_log"]
    m["pos"], m["size"] = (m["pos"] + len(out)) % cap, min(m["size"] + len(out), cap)
    return out


def copy_member(m):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}


ARRAYS = R.ARRAYS + PENDING
SCALARS = R.SCALARS


def assert_members_equal(got, want, what=""):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k, np.argwhere(a != b)[:4].tolist())


REWARDS = np.array([-0.0, 0.0, 200.0, -200.0, 0.1, 1.0 / 3.0, -7.3, 1e-3], np.float32)


def scripted_call(rng, m, call, W):
    """New inputs for call number `call` (0-based) of the 20-call script, in place -> the rows whose resetting flag the CALLER sets
    before the call.  Environment 1 ends at its first step; environment 0 ends on two consecutive calls (2, 3); the caller flags
    environment 2 before call 5; at call min(19, 6 + W) every environment ends at once (with capacity == n W the ring wraps inside
    that call); elsewhere environments >= 3 end with probability 0.15.  Rewards: -0.0f, 0, +-200 and values whose product with
    gamma^k is inexact, so that a fused multiply-add shows."""
    n, D = m["n"], m["D"]
    m["obs"][:n] = rng.standard_normal((n, D)).astype(np.float32)
    m["action"][:n] = rng.standard_normal((n, 2)).astype(np.float32)
    m["reward"][:n] = np.where(rng.random(n) < 0.7, rng.choice(REWARDS, n), rng.standard_normal(n).astype(np.float32) * 50).astype(np.float32)
    m["last_return"][:n] = (rng.integers(-8000, 8000, n) / 8.0).astype(np.float32)
    done = np.zeros(n, np.uint8)
    if n > 3:
        done[3:] = rng.random(n - 3) < 0.15
    if call == 0 and n > 1:
        done[1] = 1
    if call in (2, 3):
        done[0] = 1
    if call == min(19, 6 + W):
        done[:] = 1
    m["done"][:n] = done
    return [2] if call == 5 and n > 2 else []
