"""cn_tab_learn_act (csrc/crowdnav_tab.hip) on the GPU: the reference's sequences at n = 1, the order of reads and writes at one
wavefront, a chunk edge and two chunks plus a tail, chooseAction's branches, the documented device draw, the fused agent against its
PyTorch path on a VecEnv, the trainer, and a hipGraph.  The expectation is `Ref` of tests/tabular_ref.py: a Python loop written from
the rules in include/crowdnav.h, on a dict as the reference's, that does not call crowdnav.tabular.  Every comparison is equality.
(The tile seam, single-wavefront cells, the action range, all 1023 pairs, the epsilon memo and the refusals: test_gpu_tabular_edges.py.)"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "tabular.npz"))


# ---- the restatement: tests/tabular_ref.py ---------------------------------------------------------------------------------------
from tabular_ref import ALPHA, GAMMA, Ref, _draws, _mix, _state_table, obs_at, states_of  # noqa: E402,F401


def _agent(sarsa, **kw):
    from crowdnav import tabular
    ag = (tabular.Sarsa if sarsa else tabular.QLearn)(alpha=ALPHA, gamma=GAMMA, device=DEV, **kw)
    ag.enable_fused()
    return ag


def _seed_table(ag, ref, rng, states):
    """The same pre-launch entries in both: values for some cells of `states`."""
    for s in sorted(set(states)):
        for a in range(3):
            if rng.random() < 0.6:
                ref.q[(s, a)] = float(np.round(rng.normal(0, 5), 3))
    q, p = ref.arrays()
    ag.set_table(q, p)


def _check_table(ag, ref):
    q, p, counts = ag.table()
    rq, rp = ref.arrays()
    assert np.array_equal(p, rp)
    assert np.array_equal(q, rq)
    assert counts == (ref.same, ref.diff)


def _dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _launch_both(ag, ref, o1, a1, r, o2, keep=None, eps=0.3, rng=None, learn=True, act=True, u_learn=None, u_act=None):
    n = len(o2)
    rng = rng or np.random.default_rng(n)
    ul = rng.random((n, 5)) if u_learn is None else u_learn
    ua = rng.random((n, 5)) if u_act is None else u_act
    r32 = np.asarray(r, dtype=np.float32)
    out = ag.learn_act(_dev(o1, torch.float32) if learn else None, _dev(a1, torch.int32) if learn else None, _dev(r32, torch.float32) if learn else None,
                       _dev(o2, torch.float32), keep=_dev(keep, torch.uint8) if keep is not None else None, u_learn=ul, u_act=ua,
                       learn=learn, act=act, epsilon=eps, want=True)
    s1 = states_of(o1) if learn else None
    s2 = states_of(o2)
    acts, rows = ref.launch(s1, a1, r32.astype(np.float64) if learn else None, s2, keep, ul, ua, eps, learn, act)
    torch.cuda.synchronize()
    assert out["state"].cpu().tolist() == s2
    if learn:
        assert out["state_prev"].cpu().tolist() == s1
    if act:
        assert out["action"].cpu().tolist() == acts
        assert np.array_equal(out["q_row"].cpu().numpy(), np.array(rows))
        from crowdnav.dqn import TWISTS
        assert np.array_equal(out["twist"].cpu().numpy(), np.array(TWISTS, dtype=np.float32)[acts])
    _check_table(ag, ref)
    return out


# ---- n = 1: the reference's own sequences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["ql", "sa"])
def test_n1_golden_sequence_through_the_device(G, prefix):
    eps = float(G["hyper"][0])
    ag = _agent(prefix == "sa", epsilon=eps)
    obs = _dev(G[prefix + "_obs"], torch.float32)
    rew = _dev(G[prefix + "_reward"], torch.float32)
    ua, ul = _dev(G[prefix + "_u_act"], torch.float64), _dev(G[prefix + "_u_learn"], torch.float64)
    s = states_of(G[prefix + "_obs"])
    T = len(s) - 1
    acts = []
    out = ag.learn_act(None, None, None, obs[0:1], u_act=ua[0:1], learn=False, act=True)
    for t in range(1, T + 1):
        acts.append(out["action"])
        out = ag.learn_act(obs[t - 1:t], out["action"], rew[t - 1:t], obs[t:t + 1], u_learn=ul[t - 1:t], u_act=ua[t:t + 1] if t < T else None,
                           learn=True, act=t < T)
        if t % 20 == 0 or t == T:
            got = torch.cat(acts).cpu().numpy()
            assert np.array_equal(got, G[prefix + "_action"][:t]), t
            q, p, counts = ag.table()
            want = {}                                              # the dict after transition t, from the recorded touched entries
            for k in range(t):
                want[(s[k], int(G[prefix + "_action"][k]))] = G[prefix + "_touched"][k]
            assert {(int(i), int(a)): q[i, a] for i, a in zip(*np.nonzero(p))} == want, t
            assert sum(counts) == t
    from crowdnav import tabular
    final = {(tabular.KEY_INDEX[k.decode()], int(a)): float(v) for k, a, v in zip(G[prefix + "_q_keys"], G[prefix + "_q_actions"], G[prefix + "_q_values"])}
    q, p, counts = ag.table()
    assert {(int(i), int(a)): q[i, a] for i, a in zip(*np.nonzero(p))} == final
    assert counts == tuple(int(c) for c in G[prefix + "_counts"])


# ---- the order of reads and writes -------------------------------------------------------------------------------------------
def _case(name, n, rng):
    """-> (obs_prev, action_prev, reward, obs, keep) as double / int arrays."""
    keep = None
    a1 = rng.integers(0, 3, n)
    r = np.round(rng.normal(0, 10, n), 2)
    if name == "one_cell":                       # all rows on one cell that starts absent: the first sets, the rest blend in row order
        o1 = [obs_at(7, 18)] * n; o2 = [obs_at(7, 18)] * n; a1 = np.full(n, 1)
    elif name == "distinct":                     # all rows on distinct cells
        pairs = [(d, h) for d in range(2, 10) for h in range(12, 32)][:n]
        o1 = [obs_at(*p) for p in pairs]; o2 = [obs_at(*p) for p in reversed(pairs)]
        assert len(set(states_of(o1))) == n
    elif name == "aliased":                      # rows alternating between the two pairs of one key: one cell
        o1 = [obs_at(1, 10) if i % 2 == 0 else obs_at(11, 0) for i in range(n)]
        o2 = [obs_at(11, 0) if i % 2 == 0 else obs_at(1, 10) for i in range(n)]
        a1 = np.full(n, 2)
        assert len(set(states_of(o1))) == 1 and obs_at(1, 10) != obs_at(11, 0)
    elif name == "zero_first":                   # a reward of 0 as a cell's first write, then blends: 0.0 is a present entry
        o1 = [obs_at(3, 3 + (i % 4)) for i in range(n)]; o2 = [obs_at(3, 3 + ((i + 1) % 4)) for i in range(n)]
        a1 = np.zeros(n, dtype=np.int64); r[:4] = 0.0
    elif name == "keep_third":                   # keep masks every third row out
        o1 = [obs_at(5 + (i % 3), 20) for i in range(n)]; o2 = [obs_at(5 + ((i + 1) % 3), 20) for i in range(n)]
        keep = np.array([i % 3 != 0 for i in range(n)], dtype=np.uint8)
    elif name == "chain":                        # row i bootstraps from the state row i - 1 writes in the same launch
        o1 = [obs_at(10 + (i % 13), 5 + (i % 7)) for i in range(n)]; o2 = [o1[i - 1] for i in range(n)]
    else:
        raise KeyError(name)
    return np.array(o1), a1, r, np.array(o2), keep


@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", [64, 65, 130])
@pytest.mark.parametrize("name", ["one_cell", "distinct", "aliased", "zero_first", "keep_third"])
def test_write_order(name, n, sarsa):
    rng = np.random.default_rng(1000 * n + len(name))
    o1, a1, r, o2, keep = _case(name, n, rng)
    ag, ref = _agent(sarsa), Ref(sarsa)
    _launch_both(ag, ref, o1, a1, r, o2, keep, rng=rng)                  # from the empty table
    if name == "one_cell":
        assert (ref.same, ref.diff) == (1, n - 1)
    if name == "zero_first":
        assert ref.same == 4 and ref.diff == n - 4
    _launch_both(ag, ref, o2, a1, r[::-1].copy(), o1, keep, rng=rng)     # and again, on what the first launch left


@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("n", [64, 65, 130])
def test_bootstrap_reads_are_pre_launch(n, sarsa):
    """A row whose s2 is a cell written earlier in the same launch bootstraps from the old value: the restatement that reads the
    live table instead gives another table, so the case can tell the two orders apart."""
    rng = np.random.default_rng(77 + n)
    o1, a1, r, o2, keep = _case("chain", n, rng)
    ag, ref, wrong = _agent(sarsa), Ref(sarsa), Ref(sarsa, live_reads=True)
    _seed_table(ag, ref, np.random.default_rng(5), states_of(o1))
    wrong.q = dict(ref.q)
    ul, ua = rng.random((n, 5)), rng.random((n, 5))
    wrong.launch(states_of(o1), a1, np.asarray(r, np.float32).astype(np.float64), states_of(o2), None, ul, ua, 0.0)
    _launch_both(ag, ref, o1, a1, r, o2, None, eps=0.0, u_learn=ul, u_act=ua)
    assert ref.q != wrong.q


def test_launch_past_one_tile_and_wide_rows():
    """1 100 rows (three tiles of 512) read in place from 363-wide rows: tiles keep the ascending order."""
    n, rng = 1100, np.random.default_rng(3)
    pairs = [(int(rng.integers(0, 6)), int(rng.integers(0, 5))) for _ in range(n + 1)]
    o = np.array([obs_at(*p) for p in pairs])
    wide = np.zeros((n + 1, 363), dtype=np.float32); wide[:, 361:] = o.astype(np.float32)
    wide = torch.from_numpy(wide).to(DEV)
    a1, r = rng.integers(0, 3, n), np.round(rng.normal(0, 10, n), 2).astype(np.float32)
    ul, ua = rng.random((n, 5)), rng.random((n, 5))
    for sarsa in (False, True):
        ag, ref = _agent(sarsa), Ref(sarsa)
        out = ag.learn_act(wide[:-1], _dev(a1, torch.int32), _dev(r, torch.float32), wide[1:], u_learn=ul, u_act=ua, epsilon=0.2, want=True)
        acts, _ = ref.launch(states_of(o[:-1]), a1, r.astype(np.float64), states_of(o[1:]), None, ul, ua, 0.2)
        assert out["action"].cpu().tolist() == acts
        _check_table(ag, ref)


def test_digitize_on_the_device_every_multiple_of_a_thousandth():
    x = np.array([round(k / 1000.0, 3) for k in range(-4000, 4001)])
    o = np.stack([x, x[::-1]], 1)
    ag = _agent(False)
    out = ag.learn_act(None, None, None, _dev(o, torch.float32), learn=False, act=True, epsilon=0.0, want=True)
    assert out["state"].cpu().tolist() == states_of(o)


# ---- chooseAction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
@pytest.mark.parametrize("eps", [0.0, 1.0, 0.3])
def test_act_ties_noise_and_epsilon(sarsa, eps):
    """130 rows over: an absent state (three-way tie; under epsilon Q-learning's mag = 0 keeps it one), a two-way tie, a unique
    maximum, negative rows."""
    n, rng = 130, np.random.default_rng(int(eps * 10) + 2 * sarsa)
    ag, ref = _agent(sarsa), Ref(sarsa)
    st = {k: states_of([obs_at(*p)])[0] for k, p in dict(absent=(4, 4), two=(5, 5), uniq=(6, 6), neg=(7, 7), zero=(8, 8)).items()}
    ref.q.update({(st["two"], 0): 1.5, (st["two"], 1): 1.5, (st["two"], 2): 0.25, (st["uniq"], 0): -1.0, (st["uniq"], 2): 3.0,
                  (st["neg"], 0): -2.0, (st["neg"], 1): -2.0, (st["neg"], 2): -7.0, (st["zero"], 1): 0.0})
    q, p = ref.arrays(); ag.set_table(q, p)
    o = np.array([obs_at(*[(4, 4), (5, 5), (6, 6), (7, 7), (8, 8)][i % 5]) for i in range(n)])
    out = _launch_both(ag, ref, None, None, None, o, eps=eps, rng=rng, learn=False)
    acts = np.array(out["action"].cpu().tolist())
    if eps == 0.0:
        assert set(acts[0::5]) == {0, 1, 2} and set(acts[1::5]) == {0, 1} and set(acts[2::5]) == {2} and set(acts[3::5]) == {0, 1}
    if eps == 1.0 and not sarsa:       # mag = 0: the noise leaves the absent row at 0.0, still a three-way tie
        assert np.all(out["q_row"].cpu().numpy()[0::5] == 0.0) and set(acts[0::5]) == {0, 1, 2}
    if eps == 1.0 and sarsa:
        assert set(acts[2::5]) == {0, 1, 2}


@pytest.mark.parametrize("sarsa", [False, True])
def test_epsilon_schedule_on_the_device(sarsa):
    """episodes_dev: epsilon = the schedule applied E + 1 times, bit for bit (a draw one ulp below explores, the value itself does
    not); the handle's memo of the loop state gives the same value whatever order E comes in."""
    from crowdnav.dqn import epsilon_after
    ag = _agent(sarsa, epsilon=0.9, epsilon_discount=0.9986)
    ag.set_table(np.array([[1.0, 2.0, 3.0]] * 977), np.ones((977, 3), dtype=bool))     # greedy: action 2, no tie
    o = _dev([obs_at(9, 9)] * 3, torch.float32)
    E = torch.zeros((), dtype=torch.int64, device=DEV)
    for e in (0, 5, 700, 5, 3000, 0, 701):
        want = epsilon_after(e + 1, 0.9, 0.9986, 0.05)
        u = np.full((3, 5), 0.0)
        u[:, 0] = [np.nextafter(want, 0.0), want, np.nextafter(want, 1.0)]
        u[:, 1:4] = [0.0, 0.0, 0.99]          # SARSA explores to int(0 * 3) = 0; Q-learning's noise lifts q[0]: (1 + 0) - 1.5 < (3 + .99 * 3) - 1.5
        if not sarsa:
            u[:, 1:4] = [0.99, 0.0, 0.0]      # explores to action 0: (1 + 2.97) - 1.5 = 2.47 > (3 + 0) - 1.5
        E.fill_(e)
        out = ag.learn_act(None, None, None, o, u_act=u, learn=False, act=True, episodes_dev=E)
        assert out["action"].cpu().tolist() == [0, 2, 2], (e, want)
    assert epsilon_after(3001, 0.9, 0.9986, 0.05) <= 0.05 < epsilon_after(701, 0.9, 0.9986, 0.05)


# ---- the device draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
def test_device_draw_is_the_documented_hash(sarsa):
    n, rng = 130, np.random.default_rng(9)
    pairs = [(int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(n + 1)]
    o = np.array([obs_at(*p) for p in pairs])
    a1, r = rng.integers(0, 3, n), np.round(rng.normal(0, 10, n), 2).astype(np.float32)
    tables, actions = [], []
    for counter in (0, 12345, 12345):
        ag, ref = _agent(sarsa, seed=3), Ref(sarsa)
        ag._calls = counter
        out = ag.learn_act(_dev(o[:-1], torch.float32), _dev(a1, torch.int32), _dev(r, torch.float32), _dev(o[1:], torch.float32), epsilon=0.5)
        ul, ua = _draws(ag._seed, counter, n, 0x6a09e667f3bcc909), _draws(ag._seed, counter, n, 0xbb67ae8584caa73b)
        acts, _ = ref.launch(states_of(o[:-1]), a1, r.astype(np.float64), states_of(o[1:]), None, ul, ua, 0.5)
        assert out["action"].cpu().tolist() == acts
        _check_table(ag, ref)
        tables.append(ag.table()[0]); actions.append(acts)
    assert actions[1] == actions[2] and np.array_equal(tables[1], tables[2])
    assert actions[0] != actions[1]


# ---- the agent: fused against its PyTorch path on a VecEnv ------------------------------------------------------------------
@pytest.mark.parametrize("sarsa", [False, True])
def test_fused_agent_equals_torch_path_on_a_vecenv(sarsa):
    from crowdnav import Config, tabular
    from crowdnav.env import VecEnv
    cls = tabular.Sarsa if sarsa else tabular.QLearn
    env = VecEnv(Config(n_envs=16, n_peds=6, seed=2, max_steps=6, obs_layout=1))
    assert env.D == 363
    fused, eager = cls(epsilon=0.4, device=DEV, seed=1), cls(epsilon=0.4, device=DEV, seed=1)
    fused.enable_fused()
    rng = np.random.default_rng(4)
    obs = env.reset()
    u0 = rng.random((16, 5))
    a = fused.learn_act(None, None, None, obs, u_act=u0, learn=False)
    b = eager.learn_act(None, None, None, obs, u_act=u0, learn=False)
    resetting = torch.zeros(16, dtype=torch.bool, device=DEV)
    prev = torch.empty_like(obs)
    for it in range(8):
        assert torch.equal(a["action"], b["action"]) and torch.equal(a["twist"], b["twist"])
        prev.copy_(obs)
        obs, reward, done = env.step(a["twist"], auto_reset="next")
        keep = ~resetting
        resetting = done.bool()
        ul, ua = rng.random((16, 5)), rng.random((16, 5))
        act_prev = a["action"]
        a = fused.learn_act(prev, act_prev, reward, obs, keep=keep, u_learn=ul, u_act=ua)
        b = eager.learn_act(prev, act_prev, reward, obs, keep=keep, u_learn=ul, u_act=ua)
        qa, pa, ca = fused.table(); qb, pb, cb = eager.table()
        assert np.array_equal(pa, pb) and np.array_equal(qa, qb) and ca == cb
    assert ca[0] > 0 and ca[1] > 0 and sum(ca) < 8 * 16        # some first writes, some blends, some reset launches masked out
    env.close()


def test_trainer_end_to_end(tmp_path):
    import csv
    import glob
    from crowdnav import tabular, train
    out = str(tmp_path / "sarsa")
    agent, episodes = train.main(["--algo", "sarsa", "--envs", "16", "--launches", "60", "--learner", "fused", "--csv", "--log-every", "20",
                                  "--scenario", "training_as_logged", "--waypoint-reward", "0", "--max-steps", "10", "--out", out])
    assert episodes > 0
    rows = list(csv.reader(open(os.path.join(out, "sarsa_training.csv"))))
    assert len(rows[0]) == 8 and len(rows) == episodes + 1
    files = glob.glob(os.path.join(out, "sarsa_qtable_ep*.txt"))
    assert files == [os.path.join(out, "sarsa_qtable_ep%d.txt" % episodes)]
    loaded = tabular.Sarsa(device=DEV)
    loaded.enable_fused()
    loaded.load_q(files[0])
    q0, p0, _ = loaded.table()                                       # cn_tab_get before
    qa, pa, _ = agent.table()
    assert p0.sum() > 0 and np.array_equal(q0, qa) and np.array_equal(p0, pa)
    ev, _ = train.main(["--algo", "sarsa", "--evaluate", "--load-qtable", files[0], "--epsilon", "0", "--envs", "16", "--launches", "30",
                        "--learner", "fused", "--scenario", "training_as_logged", "--max-steps", "10", "--out", str(tmp_path / "eval")])
    q1, p1, c1 = ev.table()                                          # cn_tab_get after
    assert q1.tobytes() == q0.tobytes() and p1.tobytes() == p0.tobytes() and c1 == (0, 0)
    assert glob.glob(os.path.join(str(tmp_path / "eval"), "*qtable*")) == []


def test_graph_replay_equals_plain_calls():
    n, rng = 130, np.random.default_rng(21)
    pairs = [(int(rng.integers(0, 5)), int(rng.integers(0, 5))) for _ in range(n + 1)]
    o = _dev(np.array([obs_at(*p) for p in pairs]), torch.float32)
    o1, o2 = o[:-1].contiguous(), o[1:].contiguous()
    a1, r = _dev(rng.integers(0, 3, n), torch.int32), _dev(np.round(rng.normal(0, 10, n), 2), torch.float32)
    ul, ua = _dev(rng.random((n, 5)), torch.float64), _dev(rng.random((n, 5)), torch.float64)
    for sarsa in (False, True):
        g, plain = _agent(sarsa), _agent(sarsa)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                out = g.learn_act(o1, a1, r, o2, u_learn=ul, u_act=ua, epsilon=0.3)
        torch.cuda.current_stream().wait_stream(st)
        for k in range(2):
            graph.replay()
            want = plain.learn_act(o1, a1, r, o2, u_learn=ul, u_act=ua, epsilon=0.3)
            torch.cuda.synchronize()
            assert torch.equal(out["action"], want["action"]) and torch.equal(out["twist"], want["twist"])
        qa, pa, ca = g.table(); qb, pb, cb = plain.table()
        assert np.array_equal(qa, qb) and np.array_equal(pa, pb) and ca == cb and sum(ca) == 2 * n
