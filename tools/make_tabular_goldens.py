"""Writes tests/golden/tabular.npz from the reference's own tabular learners: turtlebot3_rl_sim/src/qlearn.py (QLearn) and sarsa.py
(Sarsa), imported unmodified with stub `rospkg` / `utils` modules in sys.modules (utils.load_q -> an empty dict: QLearn's
constructor loads a published table, the recorded sequence starts from an empty one).  random.random is a recorded stream and
random.choice is Python 2's seq[int(random() * len(seq))], the interpreter the reference ran on.

Per class, one episode-like sequence of transitions driven the way start_sarsa_training.py:74-103 drives them (chooseAction(state)
-> reward -> [SARSA: chooseAction(nextState)] -> learn -> state = nextState) over pinned observations that visit the two pairs of
an aliased key, (0, 12) next to (1, 2), a repeated cell, a reward of exactly 0 as a cell's first write, and three-way ties.
Recorded: the observations (multiples of 0.001, as the env rounds them), their (d, h) and keys, actions, rewards (float32 values),
the uniforms consumed (raw, and laid out in the five slots of crowdnav.tabular), the touched entry after every learn, the final
dict and both counters.  Also the two published discrete tables as plain arrays (key bytes, action, value) and the bin edges.

    python tools/make_tabular_goldens.py /path/to/turtlebot3_rl_sim/src
"""
import os
import pickle
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "tabular.npz")
EPSILON, ALPHA, GAMMA = 0.3, 0.2, 0.9
FILL = 0.5                                     # value of a slot the reference did not consume


def _stub_modules():
    rospkg = types.ModuleType("rospkg")

    class RosPack:
        def get_path(self, name):
            return ""
    rospkg.RosPack = RosPack
    utils = types.ModuleType("utils")
    utils.load_q = lambda path: {}
    sys.modules.update({"rospkg": rospkg, "utils": utils})


class Stream:
    """random.random(): a pinned stream that remembers what was taken."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.taken = []

    def random(self):
        u = float(self.rng.random())
        self.taken.append(u)
        return u

    def choice(self, seq):
        return seq[int(self.random() * len(seq))]

    def pop(self):
        t, self.taken = self.taken, []
        return t


def observations(rng):
    """[T + 1, 2] multiples of 0.001: the pinned walk."""
    A1, A2 = (0.050, -1.300), (1.050, -3.200)          # (1, 10) and (11, 0): both '110'
    B1, B2 = (-0.500, -0.900), (0.050, -2.800)         # (0, 12) = '012' and (1, 2) = '12'
    seq = [A1, A2] * 6 + [B1, B2] * 3
    seq += [(0.733, 0.411)] * 16                       # a repeated cell
    seq += [(2.950, 3.100), (2.950, 3.100), (0.733, 0.411), (2.950, 3.100)]     # (30, 32), fresh: its first write is reward 0
    pool = [A1, A2, B1, B2, (0.733, 0.411), (2.950, 3.100), (0.700, 0.000), (0.699, -0.001), (1.000, 1.570), (2.900, -3.140),
            (0.300, 0.790), (0.299, 0.789), (3.400, 3.140), (-0.001, -3.141)]
    while len(seq) < 201:
        seq.append(pool[int(rng.integers(len(pool)))])
    return np.array(seq, dtype=np.float64)


def slots(taken, sarsa, eps):
    """The consumed draws of one chooseAction in the five slots: 0 the epsilon test, 1-3 Q-learning's noise (1: SARSA's uniform
    choice), 4 the tie break."""
    u = np.full(5, FILL)
    u[0] = taken[0]
    rest = list(taken[1:])
    if sarsa:
        if rest:
            u[1 if taken[0] < eps else 4] = rest.pop(0)
    else:
        if taken[0] < eps:
            u[1:4] = rest[:3]
            rest = rest[3:]
        if rest:
            u[4] = rest.pop(0)
    assert not rest, taken
    return u


def record(cls_mod, cls_name, sarsa, seed, distance_bins, radian_bins):
    st = Stream(seed)
    cls_mod.random.random = st.random
    cls_mod.random.choice = st.choice
    agent = getattr(cls_mod, cls_name)(actions=range(3), epsilon=EPSILON, alpha=ALPHA, gamma=GAMMA)
    rng = np.random.default_rng(seed + 1)
    obs = observations(rng)
    T = len(obs) - 1
    d = np.array([int(np.digitize([o[0]], distance_bins)[0]) for o in obs])
    h = np.array([int(np.digitize([o[1]], radian_bins)[0]) for o in obs])
    keys = ["".join(map(str, (a, b))) for a, b in zip(d, h)]            # start_sarsa_training.py:70-72
    reward = rng.normal(0.0, 10.0, T).astype(np.float32).astype(np.float64)
    reward[::7] = np.round(reward[::7])                                  # some integer rewards, as the env's mostly are
    first30 = keys.index("3032")
    reward[first30] = 0.0                                                # a cell's first write is exactly 0 ...
    reward[first30 + 1] = -3.5                                           # ... and the same state is stepped again
    act, a2s, touched = np.zeros(T, np.int64), np.full(T, -1, np.int64), np.zeros(T)
    u_act, u_learn = np.full((T, 5), FILL), np.full((T, 5), FILL)
    n_act, n_learn, raw = np.zeros(T, np.int64), np.zeros(T, np.int64), []
    for t in range(T):
        state, nxt = keys[t], keys[t + 1]
        a = agent.chooseAction(state)
        tk = st.pop(); raw += tk; n_act[t] = len(tk); u_act[t] = slots(tk, sarsa, EPSILON)
        if sarsa:
            a2 = agent.chooseAction(nxt)
            tk = st.pop(); raw += tk; n_learn[t] = len(tk); u_learn[t] = slots(tk, True, EPSILON)
            agent.learn(state, a, float(reward[t]), nxt, a2)
            a2s[t] = a2
        else:
            agent.learn(state, a, float(reward[t]), nxt)
        act[t] = a
        touched[t] = agent.q[(state, a)]
    items = sorted(agent.q.items())
    same_first = reward[first30] == 0.0 and ("3032", int(act[first30])) in agent.q
    assert same_first
    return dict(obs=obs, dh=np.stack([d, h], 1), keys=np.array(keys, dtype="S4"), action=act, reward=reward, a2=a2s, touched=touched,
                u_act=u_act, u_learn=u_learn, n_act=n_act, n_learn=n_learn, raw=np.array(raw),
                q_keys=np.array([k[0] for k, _ in items], dtype="S4"), q_actions=np.array([k[1] for k, _ in items], dtype=np.int64),
                q_values=np.array([v for _, v in items], dtype=np.float64), counts=np.array([agent.count_same, agent.count_diff], dtype=np.int64))


def published(path):
    with open(path, "rb") as f:
        q = pickle.load(f, encoding="latin1")
    items = sorted(q.items())
    return dict(keys=np.array([k[0] for k, _ in items], dtype="S4"), actions=np.array([k[1] for k, _ in items], dtype=np.int64),
                values=np.array([v for _, v in items], dtype=np.float64))


def main(src):
    _stub_modules()
    sys.path.insert(0, src)
    import qlearn
    import sarsa
    distance_bins = [round(i, 2) for i in np.arange(0, 3, 0.1)]                 # start_sarsa_training.py:41-45
    radian_bins = [round(i, 2) for i in np.arange(-3.14, 3.14, 0.19625)]
    out = dict(distance_bins=np.array(distance_bins), radian_bins=np.array(radian_bins),
               hyper=np.array([EPSILON, ALPHA, GAMMA]), fill=np.array(FILL))
    for prefix, mod, name, is_sarsa, seed in (("ql", qlearn, "QLearn", False, 3000), ("sa", sarsa, "Sarsa", True, 1500)):
        out.update({"%s_%s" % (prefix, k): v for k, v in record(mod, name, is_sarsa, seed, distance_bins, radian_bins).items()})
    for prefix, rel in (("pub_ql", "models/qlearn/discrete_no_greedy/qlearn_qtable_ep3000.txt"),
                        ("pub_sa", "models/sarsa/discrete/sarsa_qtable_ep1500.txt")):
        out.update({"%s_%s" % (prefix, k): v for k, v in published(os.path.join(src, rel)).items()})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items() if k.endswith(("_raw", "_keys", "counts"))})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_SRC", "turtlebot3_rl_sim/src"))
