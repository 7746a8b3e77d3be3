"""crowdnav.tabular (the PyTorch / NumPy restatement of qlearn.py and sarsa.py) against the goldens recorded from the reference's
own classes (tools/make_tabular_goldens.py -> tests/golden/tabular.npz).  Every comparison is equality: the order of reads and
writes and every rounding are pinned."""
import os
import pickle

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "tabular.npz"))


def _dict_of(G, prefix):
    return {(k.decode(), int(a)): float(v) for k, a, v in zip(G[prefix + "_keys"], G[prefix + "_actions"], G[prefix + "_values"])}


def test_key_table_and_bins(G):
    from crowdnav import tabular as T
    assert T.N_STATES == 977 == len(T.KEYS) == len(set(T.KEYS)) and T.STATE_OF.shape == (31, 33)
    assert T.STATE_OF.min() == 0 and T.STATE_OF.max() == 976
    pairs_of = {}
    for d in range(31):
        for h in range(33):
            assert T.KEYS[T.STATE_OF[d, h]] == str(d) + str(h)
            pairs_of.setdefault(int(T.STATE_OF[d, h]), []).append((d, h))
    assert sum(1 for v in pairs_of.values() if len(v) == 2) == 46 and max(len(v) for v in pairs_of.values()) == 2
    assert T.STATE_OF[1, 10] == T.STATE_OF[11, 0] and T.KEYS[T.STATE_OF[1, 10]] == "110"
    assert T.STATE_OF[0, 12] != T.STATE_OF[1, 2] and T.KEYS[T.STATE_OF[0, 12]] == "012" and T.KEYS[T.STATE_OF[1, 2]] == "12"
    # numbered in order of first appearance, d ascending then h ascending
    flat = T.STATE_OF.reshape(-1)
    firsts = [int(s) for i, s in enumerate(flat) if s not in flat[:i]]
    assert firsts == list(range(977))
    assert np.array_equal(T.DISTANCE_BINS, G["distance_bins"]) and len(T.DISTANCE_BINS) == 30
    assert np.array_equal(T.RADIAN_BINS, G["radian_bins"]) and len(T.RADIAN_BINS) == 32


def test_digitize_float32_equals_numpy_on_the_double(G):
    from crowdnav import tabular as T
    x = np.array([round(k / 1000.0, 3) for k in range(-4000, 4001)], dtype=np.float64)
    assert len(x) == 8001
    for bins in (G["distance_bins"], G["radian_bins"]):
        want = np.digitize(x, bins)
        assert np.array_equal(T.digitize(x.astype(np.float32), bins), want)
        assert np.array_equal(T.digitize(x, bins), want)
        assert not np.array_equal(np.digitize(x.astype(np.float32).astype(np.float64), bins), want)    # why the edges are narrowed
    obs = np.stack([x, x[::-1]], 1)
    d, h, s = T.digitize_state(obs.astype(np.float32), return_dh=True)
    assert np.array_equal(d, np.digitize(x, G["distance_bins"])) and np.array_equal(h, np.digitize(x[::-1], G["radian_bins"]))
    assert np.array_equal(s, T.STATE_OF[d, h]) and np.array_equal(T.digitize_state(obs), s)
    wide = np.zeros((5, 363), dtype=np.float32); wide[:, -2:] = obs[3000:3005]
    assert np.array_equal(T.digitize_state(wide), s[3000:3005])


@pytest.mark.parametrize("prefix", ["ql", "sa"])
def test_n1_replays_the_reference_sequence(G, prefix):
    from crowdnav import tabular as T
    eps, alpha, gamma = (float(v) for v in G["hyper"])
    ag = (T.QLearn if prefix == "ql" else T.Sarsa)(epsilon=eps, alpha=alpha, gamma=gamma)
    obs, keys = G[prefix + "_obs"], G[prefix + "_keys"]
    d, h, s = T.digitize_state(obs.astype(np.float32), return_dh=True)
    assert np.array_equal(np.stack([d, h], 1), G[prefix + "_dh"])
    assert [T.KEYS[i] for i in s] == [k.decode() for k in keys]
    assert len({b"110"} & set(keys)) == 1 and {(1, 10), (11, 0)} <= {tuple(r) for r in G[prefix + "_dh"]}     # the aliased pair is visited
    n = len(obs) - 1
    for t in range(n):
        o, o2 = obs[t:t + 1].astype(np.float32), obs[t + 1:t + 2].astype(np.float32)
        a = ag.chooseAction(o, u=G[prefix + "_u_act"][t:t + 1])
        assert int(a[0]) == int(G[prefix + "_action"][t]), t
        ag.learn(o, a, np.float32(G[prefix + "_reward"][t]).reshape(1), o2, u=G[prefix + "_u_learn"][t:t + 1])
        assert ag.getQ(s[t], int(a[0])) == G[prefix + "_touched"][t], t
    assert ag.get_qtable() == _dict_of(G, prefix + "_q")
    assert (ag.count_same, ag.count_diff) == tuple(int(c) for c in G[prefix + "_counts"])


def test_sarsa_next_action_is_the_references(G):
    """The a2 the learn phase draws (chooseAction(s2) on the pre-write table) is the reference's nextAction."""
    from crowdnav import tabular as T
    eps, alpha, gamma = (float(v) for v in G["hyper"])
    ag = T.Sarsa(epsilon=eps, alpha=alpha, gamma=gamma)
    obs = G["sa_obs"].astype(np.float32)
    s = T.digitize_state(obs)
    for t in range(len(obs) - 1):
        a2, _ = T.choose(ag.table()[0], s[t + 1:t + 2], G["sa_u_learn"][t:t + 1], eps, True)
        assert int(a2[0]) == int(G["sa_a2"][t]), t
        ag.learn(obs[t:t + 1], G["sa_action"][t:t + 1], G["sa_reward"][t:t + 1], obs[t + 1:t + 2], u=G["sa_u_learn"][t:t + 1])


def test_batched_order_one_cell_and_prelaunch_reads():
    """n rows on one cell: the first sets, the rest blend in row order; every bootstrap read is from the table before the call."""
    from crowdnav import tabular as T
    ag = T.QLearn(epsilon=0.0, alpha=0.2, gamma=0.9)
    o = np.tile(np.array([[0.733, 0.411]], dtype=np.float32), (5, 1))
    r = np.array([2.0, 0.0, -1.0, 4.0, 8.0], dtype=np.float32)
    ag.learn(o, np.zeros(5, dtype=np.int64), r, o)
    want = 2.0
    for x in r[1:]:
        want = want + 0.2 * ((float(x) + 0.9 * 0.0) - want)          # s2 is the cell itself: its bootstrap stays the pre-call 0.0
    s = int(T.digitize_state(o)[0])
    assert ag.getQ(s, 0) == want and (ag.count_same, ag.count_diff) == (1, 4)
    q, p, _ = ag.table()
    assert p.sum() == 1 and np.count_nonzero(q) == 1


def test_load_save_round_trip(G, tmp_path):
    from crowdnav import tabular as T
    for prefix, cls in (("pub_ql", T.QLearn), ("pub_sa", T.Sarsa)):
        d = _dict_of(G, prefix)
        assert len(d) == (992 if prefix == "pub_ql" else 1365)
        src = tmp_path / (prefix + ".txt")
        with open(src, "wb") as f:
            pickle.dump(d, f, protocol=2)
        ag = cls()
        ag.load_q(str(src))
        assert ag.get_qtable() == d and (ag.count_same, ag.count_diff) == (0, 0)
        path = ag.save(str(tmp_path), 1500)
        assert os.path.basename(path) == "%s_qtable_ep1500.txt" % ("qlearn" if cls is T.QLearn else "sarsa")
        raw = open(path, "rb").read()
        assert raw[:2] == b"\x80\x02"                                  # pickle protocol 2
        back = pickle.loads(raw)
        assert back == d and all(type(k[0]) is str and type(k[1]) is int and type(v) is float for k, v in back.items())
        ag2 = cls(); ag2.load_q(path)
        q1, p1, _ = ag.table(); q2, p2, _ = ag2.table()
        assert np.array_equal(q1, q2) and np.array_equal(p1, p2)
    for bad in ({("0.733", 0): 1.0}, {("3133", 0): 1.0}, {("110", 3): 1.0}, {"110": 1.0}):      # unbinned decimals: the `continuous` tables
        src = tmp_path / "bad.txt"
        with open(src, "wb") as f:
            pickle.dump(bad, f, protocol=2)
        with pytest.raises(ValueError, match="discrete"):
            T.QLearn().load_q(str(src))


def test_device_draws_are_uniforms_keyed_by_counter_row_and_slot():
    from crowdnav import tabular as T
    a, b = T.device_draws(7, 3, 130, "act"), T.device_draws(7, 3, 130, "act")
    assert a.shape == (130, 5) and np.array_equal(a, b) and a.min() >= 0.0 and a.max() < 1.0
    assert not np.array_equal(a, T.device_draws(7, 4, 130, "act")) and not np.array_equal(a, T.device_draws(7, 3, 130, "learn"))
    assert len(np.unique(a)) == a.size
    # splitmix64's finaliser on a known input
    assert int(T._mix64(np.array([0], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_parse_args_defaults_and_rejected_flags():
    from crowdnav import train
    for algo, out in (("qlearn", "runs/qlearn"), ("sarsa", "runs/sarsa")):
        a = train.parse_args(["--algo", algo])
        assert (a.max_steps, a.obs_layout, a.reset_mode, a.out) == (200, 1, "next", out)
        assert (a.alpha, a.gamma, a.epsilon, a.epsilon_discount) == (0.2, 0.9, 0.9, 0.9986)
        assert a.load_qtable is None and not a.evaluate
        for flag in (["--updates", "4"], ["--memory", "1000"], ["--batch", "64"], ["--graphs", "1"], ["--reset-mode", "same"]):
            with pytest.raises(SystemExit):
                train.parse_args(["--algo", algo] + flag)
        b = train.parse_args(["--algo", algo, "--epsilon", "0", "--alpha", "0.5", "--gamma", "0.8", "--max-steps", "50", "--evaluate",
                              "--load-qtable", "x.txt"])
        assert (b.epsilon, b.alpha, b.gamma, b.max_steps, b.evaluate, b.load_qtable) == (0.0, 0.5, 0.8, 50, True, "x.txt")
    # the other learners keep their defaults
    a = train.parse_args(["--algo", "dqn"])
    assert (a.epsilon, a.epsilon_discount, a.max_steps, a.updates, a.memory, a.graphs) == (1.0, 0.995, 250, 4, 1_000_000, 1)
    a = train.parse_args([])
    assert (a.algo, a.max_steps, a.updates) == ("td3", 1000, 4)
