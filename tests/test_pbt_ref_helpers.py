"""The NumPy restatement of cn_td3_pop_exploit (tests/pbt_ref.py) against the properties its statement promises, without a GPU: the
survivors and the replaced are disjoint, every source is a survivor, the plan is a function of (seed, calls), NaN ranks last, ties go
to the lower index, the skip rule, the clamp, and both factors over 64 draws."""
import numpy as np
import pytest

import pbt_ref as R

NAN = float("nan")


def test_mix64_is_splitmix64s_finaliser():
    # splitmix64 seeded with 0 yields 0xE220A8397B1DCDAF first: its state after one step is the increment, which mix64 adds itself
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert all(0 <= R.mix64(x) <= R.M64 for x in (R.M64, 1 << 63, 12345))


@pytest.mark.parametrize("P,n", [(2, 1), (5, 2), (7, 3), (64, 32), (64, 1)])
def test_survivors_and_replaced_are_disjoint_and_every_source_survives(P, n):
    rng = np.random.default_rng(P * 100 + n)
    for calls in range(8):
        f = rng.standard_normal(P).astype(np.float32)
        f[rng.integers(0, P, 3)] = f[0]                       # some ties
        order = R.rank(f)
        pairs = R.plan(f, n, seed=77, calls=calls)
        dst, src = [d for d, _ in pairs], [s for _, s in pairs]
        assert len(set(dst)) == n and dst == order[::-1][:n]  # the n last, worst first
        assert set(src) <= set(order[:n]) and not set(src) & set(dst)


def test_plan_is_a_function_of_seed_and_calls():
    f = np.arange(16, dtype=np.float32)
    base = R.plan(f, 8, seed=5, calls=3)
    assert base == R.plan(f.copy(), 8, seed=5, calls=3)
    others = [R.plan(f, 8, seed=s, calls=c) for s, c in ((6, 3), (5, 4), (5, 0), (1 << 63, 3))]
    assert all(o != base for o in others)
    assert [d for d, _ in base] == [d for d, _ in others[0]]  # who is replaced depends on the fitness alone


def test_nan_ranks_last_ties_go_to_the_lower_index_and_zeros_are_equal():
    assert R.rank([1.0, NAN, 3.0, NAN, 2.0]) == [2, 4, 0, 1, 3]
    assert R.rank([2.0, 2.0, 2.0]) == [0, 1, 2]
    assert R.rank([0.0, -0.0, 1.0, -0.0]) == [2, 0, 1, 3]
    assert R.rank([-0.0, 0.0]) == [0, 1]
    assert R.rank([NAN, NAN]) == [0, 1]
    assert R.rank([-np.inf, NAN, np.inf]) == [2, 0, 1]


def test_skip_rule_and_fitness_from_totals():
    cfg = R.make_config(1, min_episodes=3, seed=1)
    st = R.make_state([[1e-3, 1e-3, 0.99, 0.2, 0.5]] * 3)
    tot = np.zeros((3, 5))
    tot[:, 0], tot[:, 2] = (3, 2, 5), (30.0, 10.0, -5.0)
    keep = {k: np.copy(v) for k, v in st.items()}
    assert R.exploit(st, cfg, tot=tot) is None                # member 1 has two new episodes
    assert st["calls"] == 1 and st["applied"] == 0
    for k in ("src", "generation", "fitness", "hyper", "last"):
        assert np.array_equal(st[k], keep[k]), k
    tot[1, 0] = 3
    pairs = R.exploit(st, cfg, tot=tot)
    assert pairs == [(2, 0)] and st["calls"] == 2 and st["applied"] == 1
    assert st["fitness"].tolist() == [10.0, np.float32(10.0 / 3.0), -1.0]
    assert st["fitness"][1] == np.float32(np.float64(10.0) / np.float64(3.0))         # float64 quotient, then rounded
    assert st["last"].tolist() == [[3.0, 30.0], [3.0, 10.0], [5.0, -5.0]]
    assert R.exploit(st, cfg, tot=tot) is None and st["calls"] == 3                   # no new episodes since
    tot[:, 0] += 3
    tot[:, 2] += (0.0, 6.0, 3.0)
    assert R.exploit(st, cfg, tot=tot) is not None
    assert st["fitness"].tolist() == [0.0, 2.0, 1.0]                                  # of the NEW episodes only


def test_clamp_and_unmasked_hyper_parameters():
    src = np.array([1e-3, 2e-3, 0.99, 0.2, 0.5], np.float32)
    cfg = R.make_config(1, explore=R.HYPERS, factor=(0.5, 2.0), lo=[9e-4, 0, 0.98, 0.15, 0.4], hi=[1.1e-3, 1, 0.995, 0.3, 0.6])
    for dst in range(8):
        out = R.explore(src, dst, cfg, calls=dst)
        assert out.dtype == np.float32
        assert out[0] in (np.float32(9e-4), np.float32(1.1e-3)) and out[2] in (np.float32(0.98), np.float32(0.995))   # both clamps
        assert out[1] in (np.float32(src[1] * np.float32(0.5)), np.float32(src[1] * np.float32(2.0)))                  # inside: the product
    none = R.make_config(1, explore=0, lo=[0] * 5, hi=[1] * 5)
    assert np.array_equal(R.explore(src, 3, none, 9), src)
    only = R.make_config(1, explore=("gamma",), factor=(0.5, 0.5), lo=[0] * 5, hi=[1] * 5)
    assert R.explore(src, 3, only, 9).tolist() == [src[0], src[1], np.float32(0.495), src[3], src[4]]
    clamp_unmasked = R.make_config(1, explore=0, lo=[0, 0, 0, 0.25, 0], hi=[1] * 5)   # the clamp applies to inherited values too
    assert R.explore(src, 0, clamp_unmasked, 0)[3] == np.float32(0.25)


def test_both_factors_occur_over_64_draws():
    cfg = R.make_config(1, explore=R.HYPERS, factor=(0.5, 2.0), lo=[0] * 5, hi=[1e9] * 5, seed=11)
    src = np.ones(5, np.float32)
    seen = {float(R.explore(src, dst, cfg, calls)[k]) for dst in range(4) for calls in range(4) for k in range(4)}
    assert seen == {0.5, 2.0}
    counts = sum(R.explore(src, dst, cfg, 0)[0] == 2.0 for dst in range(64))
    assert 16 <= counts <= 48                                  # a fair bit: 64 draws miss this band with probability < 1e-4


def test_exploit_updates_the_state_as_stated():
    cfg = R.make_config(2, explore=("lr_actor",), factor=(0.5, 2.0), lo=[0] * 5, hi=[1] * 5, seed=3)
    hyp = np.array([[1e-3 * (p + 1), 1e-3, 0.99, 0.2, 0.5] for p in range(5)], np.float32)
    st = R.make_state(hyp)
    pairs = R.exploit(st, cfg, fitness=[5.0, 1.0, 4.0, NAN, 2.0])
    assert [d for d, _ in pairs] == [3, 1] and {s for _, s in pairs} <= {0, 2}
    for dst, src in pairs:
        assert st["src"][dst] == src and st["generation"][dst] == 1
        assert st["hyper"][dst][0] in (np.float32(hyp[src][0] * np.float32(0.5)), np.float32(hyp[src][0] * np.float32(2.0)))
        assert np.array_equal(st["hyper"][dst][1:], hyp[src][1:])
    for p in (0, 2, 4):
        assert st["src"][p] == p and st["generation"][p] == 0 and np.array_equal(st["hyper"][p], hyp[p])
    assert np.isnan(st["fitness"][3]) and st["fitness"][0] == 5.0
