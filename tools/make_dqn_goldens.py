"""Writes tests/golden/dqn.npz from the reference's own DQN classes: turtlebot3_rl_sim/src/deepq.py (DeepQ.learnOnMiniBatch,
selectAction) and memory.py (Memory), imported unmodified with stub `keras` / `tensorflow` modules in sys.modules.  The model is
a recorder: a float64 numpy `predict` of the 3-layer ReLU network and a `fit` that keeps what it was handed (X_batch, Y_batch,
batch_size).  random.sample is pinned (Python 3.10 rejects memory.py's ndarray population), and so are selectAction's draws.

    python tools/make_dqn_goldens.py /path/to/turtlebot3_rl_sim/src
"""
import os
import sys
import types

import numpy as np

D, H, A, B, N = 12, 16, 3, 8, 40          # inputs, hidden, actions, mini-batch, replay rows
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "dqn.npz")


def _stub_modules():
    class _Any:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, name):
            return _Any()

        def __call__(self, *a, **k):
            return _Any()
    tf = types.ModuleType("tensorflow")
    tf.ConfigProto = _Any
    tf.Session = _Any
    tk = types.ModuleType("tensorflow.keras")
    tk.Sequential = _Any
    tk.optimizers = _Any()
    layers = types.ModuleType("tensorflow.keras.layers")
    for n in ("Dense", "Activation", "LeakyReLU", "Dropout"):
        setattr(layers, n, _Any)
    models = types.ModuleType("tensorflow.keras.models")
    models.load_model = _Any
    reg = types.ModuleType("tensorflow.keras.regularizers")
    reg.l2 = _Any
    keras = types.ModuleType("keras")
    keras.models = _Any()
    tf.keras = tk
    sys.modules.update({"tensorflow": tf, "tensorflow.keras": tk, "tensorflow.keras.layers": layers, "tensorflow.keras.models": models,
                        "tensorflow.keras.regularizers": reg, "keras": keras})


class Recorder:
    def __init__(self, p):
        self.p = p
        self.fits = []

    def predict(self, x):
        p = self.p
        h1 = np.maximum(x @ p["w1"].T + p["b1"], 0.0)
        h2 = np.maximum(h1 @ p["w2"].T + p["b2"], 0.0)
        return h2 @ p["w3"].T + p["b3"]

    def fit(self, X, Y, batch_size=None, epochs=None, verbose=None):
        self.fits.append((np.array(X), np.array(Y), batch_size))


def _params(rng):
    return dict(w1=rng.uniform(-0.5, 0.5, (H, D)), b1=rng.uniform(-0.1, 0.1, H), w2=rng.uniform(-0.4, 0.4, (H, H)),
                b2=rng.uniform(-0.1, 0.1, H), w3=rng.uniform(-0.4, 0.4, (A, H)), b3=rng.uniform(-0.1, 0.1, A))


def main(src):
    _stub_modules()
    sys.path.insert(0, src)
    import deepq
    import memory
    rng = np.random.default_rng(1500)
    p, pt = _params(rng), _params(rng)
    dq = deepq.DeepQ(D, A, 1000, 0.99, 2.5e-4, B)
    dq.model, dq.targetModel = Recorder(p), Recorder(pt)
    S = rng.uniform(0, 3.5, (N, D)); S2 = rng.uniform(0, 3.5, (N, D))
    act = rng.integers(0, A, N); rew = rng.normal(0, 10, N); fin = rng.random(N) < 0.25
    for i in range(N):
        dq.addMemory(S[i], int(act[i]), float(rew[i]), S2[i], bool(fin[i]))
    out = dict(w=np.array([D, H, A, B]), S=S, S2=S2, act=act, rew=rew, fin=fin.astype(np.uint8))
    out.update({"p_" + k: v for k, v in p.items()}); out.update({"pt_" + k: v for k, v in pt.items()})
    for case, use_target in (("online", False), ("target", True)):
        idx = rng.choice(N, B, replace=False)
        memory.random.sample = lambda population, k, _i=list(idx): list(_i)[:k]
        dq.learnOnMiniBatch(B, use_target)
        X, Y, bs = (dq.model.fits[-1])
        out[case + "_idx"] = idx; out[case + "_X"] = X; out[case + "_Y"] = Y; out[case + "_bs"] = np.array(bs)
    # selectAction on pinned draws: random.random() -> u, np.random.randint -> pick
    us = np.array([0.01, 0.5, 0.99, 0.3, 0.06, 0.7]); picks = np.array([2, 1, 0, 1, 2, 0]); eps = 0.4
    qv = dq.model.predict(S[:6])
    sel = []
    for i in range(6):
        deepq.random.random = lambda _u=us[i]: float(_u)
        deepq.np.random.randint = lambda lo, hi, _k=picks[i]: int(_k)
        sel.append(int(dq.selectAction(qv[i], eps)))
    out.update(sel_u=us, sel_pick=picks, sel_eps=np.array(eps), sel_action=np.array(sel))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_SRC", "turtlebot3_rl_sim/src"))
