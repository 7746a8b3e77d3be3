"""The NumPy restatement of cn_nstep_record (tests/nstep_ref.py), which tests/test_gpu_nstep_record.py holds the kernels to, held to
what an n-step recorder must do: hand-written episodes, a derived rounding bound against float64, W = 1 as a plain masked ring
write, and the library's cn_nstep_discount (host code: no device) against the restatement's products."""
import numpy as np
import pytest

import nstep_ref as N
import pop_record_ref as R
from learner_handle import lib


def _one_env(W, gamma, D=2, cap=64):
    m = R.make_member(np.random.default_rng(0), 1, D, cap=cap, done="none", resetting="none")
    return N.add_pending(m, W, gamma)


def _episode(m, rewards, first_obs, rng, done_at_end=True):
    """One environment through len(rewards) calls -> (the emitted rows per call, the observations o_0 ... o_T, the actions)."""
    T = len(rewards)
    obs = [first_obs] + [rng.standard_normal(m["D"]).astype(np.float32) for _ in range(T)]
    acts = [rng.standard_normal(2).astype(np.float32) for _ in range(T)]
    m["prev"][0] = obs[0]
    per_call = []
    for t in range(T):
        m["action"][0], m["reward"][0], m["obs"][0] = acts[t], rewards[t], obs[t + 1]
        m["done"][0] = 1 if (done_at_end and t == T - 1) else 0
        per_call.append(N.record(m, t + 1))
        assert np.array_equal(m["prev"][0], obs[t + 1]) and m["resetting"][0] == m["done"][0]
    return per_call, obs, acts


def test_hand_written_episode_window_three():
    """W = 3, gamma = 1/2 (every product exact), rewards 1, 2, 4, 8, the episode ends with the fourth: calls 1 and 2 emit nothing, call 3
    the full-window row of step 0 with d = 0, call 4 the rows of steps 1, 2, 3, oldest first, all with d = 1 and s2 = the terminal
    observation."""
    m = _one_env(3, 0.5)
    rng = np.random.default_rng(1)
    calls, obs, acts = _episode(m, [1.0, 2.0, 4.0, 8.0], rng.standard_normal(2).astype(np.float32), rng)
    assert [len(c) for c in calls] == [0, 0, 1, 3]
    rows = calls[2] + calls[3]
    assert [float(r[3]) for r in rows] == [1 + 1 + 1, 2 + 2 + 2, 4 + 4, 8]
    assert [float(r[5]) for r in rows] == [0, 1, 1, 1]
    for i, r in enumerate(rows):
        assert np.array_equal(r[1], obs[i]) and np.array_equal(r[2], acts[i])                       # (s_i, a_i), in start order
        assert np.array_equal(r[4], obs[3] if i == 0 else obs[4])                                   # s2: three steps on / the terminal one
    assert m["pos"] == 4 and m["size"] == 4 and m["count"][0] == 0 and m["clock"][0] == 0
    assert np.array_equal(m["r"][:4], np.array([3, 6, 8, 8], np.float32)) and np.array_equal(m["d"][:4], np.array([0, 1, 1, 1], np.float32))
    assert (m["s"][4:64] != R.SENTINEL).all() and (m["s"][64:] == R.SENTINEL).all()                  # nothing beyond what was emitted
    # the reset launch that follows is not a transition: nothing is pushed, nothing emitted, the store stays empty
    before = N.copy_member(m)
    m["done"][0] = 0
    assert N.record(m, 5) == [] and m["count"][0] == 0 and m["pos"] == 4 and m["resetting"][0] == 0
    assert m["tot"][4] == before["tot"][4]
    # ... and the next episode starts a fresh window
    calls, _, _ = _episode(m, [16.0, 32.0], m["prev"][0].copy(), rng, done_at_end=False)
    assert [len(c) for c in calls] == [0, 0] and m["count"][0] == 2 and list(m["pret"][0, :2]) == [32.0, 32.0]


def test_an_episode_that_ends_at_its_first_step_and_negative_zero():
    m = _one_env(3, 0.99)
    rng = np.random.default_rng(2)
    calls, obs, _ = _episode(m, [np.float32(-0.0)], rng.standard_normal(2).astype(np.float32), rng)
    (row,) = calls[0]
    assert np.signbit(row[3]) and row[3] == 0 and row[5] == 1 and np.signbit(m["r"][0])               # assigned, not 0 + r
    assert not m["ps"].any() and not m["pret"].any()                                                   # emitted straight from prev


@pytest.mark.parametrize("W", (1, 2, 3, 5, 16))
@pytest.mark.parametrize("gamma", (0.99, 0.9, 1.0))
def test_every_return_is_within_the_derived_bound_of_the_float64_sum(W, gamma):
    """With u = 2^-24 and M = sum_k gamma^k |r_k| over the row's span (gamma as float32, the value the library is given): the first
    term is assigned (exact); term k >= 1 carries the rounding of w[k] to float32 (the float64 running product's own error, k 2^-53, is
    negligible) and the rounding of the product, each at most u gamma^k |r_k| (1 + u), together at most 2 u M (1 + u) over the row;
    each of the at most W - 1 sums is rounded once, by at most u times a partial sum whose magnitude is at most M (1 + W u).  Total:
    at most (W + 1) u M (1 + O(W u)), which is below 2 W u M for every W >= 2; for W = 1 the row is exact.  A derived bound, not a
    measured one.  Rows, their order, their spans and d are checked along the way."""
    rng = np.random.default_rng(W * 7 + int(gamma * 100))
    T = 23
    rewards = np.where(rng.random(T) < 0.5, rng.choice(N.REWARDS, T), rng.standard_normal(T) * 50).astype(np.float32)
    m = _one_env(W, gamma)
    calls, obs, acts = _episode(m, list(rewards), rng.standard_normal(2).astype(np.float32), rng)
    rows = [r for c in calls for r in c]
    assert len(rows) == T and [len(c) for c in calls[:W - 1]] == [0] * min(W - 1, T - 1)
    g = float(np.float32(gamma))
    for i, r in enumerate(rows):
        span = min(W, T - i)
        exact = sum(g ** k * float(rewards[i + k]) for k in range(span))
        mag = sum(g ** k * abs(float(rewards[i + k])) for k in range(span))
        assert abs(float(r[3]) - exact) <= 2 * W * 2.0 ** -24 * mag, (i, float(r[3]), exact)
        assert np.array_equal(r[1], obs[i]) and np.array_equal(r[2], acts[i]) and np.array_equal(r[4], obs[i + span])
        assert float(r[5]) == (1.0 if i + W - 1 >= T - 1 else 0.0)


def test_window_one_is_a_plain_masked_ring_write():
    """W = 1 against pop_record_ref.record (cn_pop_record's restatement) over three calls with every keep / done pattern mixed: all of
    ring, log, prev and resetting, byte for byte, and nothing ever pends."""
    rng = np.random.default_rng(4)
    base = R.make_member(rng, 70, 3, cap=75, pos=73, size=40, done="alternating", resetting="last")
    a, b = N.add_pending(R.copy_member(base), 1, 0.99), R.copy_member(base)
    for launch in (1, 2, 3):
        N.record(a, launch); R.record(b, launch)
        R.assert_members_equal(a, b, "launch %d" % launch)
        assert not a["ps"].any() and not a["count"].any()
        for m in (a, b):
            m["obs"][:70] = np.random.default_rng(launch).standard_normal((70, 3)).astype(np.float32)
            m["done"][:70] = R.pattern("all" if launch == 1 else "last", 70)


def test_library_discount_equals_the_restatement():
    _abi, L = lib()
    assert "cn_nstep_discount" in _abi.EXPORTS and _abi.CN_NSTEP_MAX == N.NSTEP_MAX == 16
    for gamma in (0.99, 0.9, 1.0):
        for k in range(17):
            got = np.float32(L.cn_nstep_discount(gamma, k))
            assert got.tobytes() == N.discount(gamma, k).tobytes(), (gamma, k)
        assert np.float32(L.cn_nstep_discount(gamma, 1)) == np.float32(gamma) and L.cn_nstep_discount(gamma, 0) == 1.0


def test_the_script_reaches_every_case():
    """nstep_ref.scripted_call, on the restatement alone: consecutive dones, a first-step done, the caller's flag, the all-done call
    that wraps a ring of exactly n W rows, rows with d = 0 and d = 1, a -0.0f return in the ring."""
    for W in (2, 3, 5, 16):
        m = N.add_pending(R.make_member(np.random.default_rng(W), 7, 1, cap=7 * W, pos=3, size=2, done="none", resetting="none"), W, 0.99)
        rng = np.random.default_rng(W + 1)
        emitted, wrapped = 0, False
        for call in range(20):
            for e in N.scripted_call(rng, m, call, W):
                m["resetting"][e] = 1
            pos = m["pos"]
            out = N.record(m, call + 1)
            wrapped |= call == min(19, 6 + W) and pos + len(out) > m["cap"] and len(out) >= 7
            emitted += len(out)
        assert wrapped and emitted >= 7 * W and m["size"] == m["cap"]
        d = m["d"][:m["cap"]]
        assert (d == 0).any() and (d == 1).any()
