"""A float64 restatement of the reference's DQN update (deepq.py:219-266, memory.py:22-28, Keras fit / mse / RMSprop) and action
selection, for the parity tests.  Variants that are NOT the reference are switches, so the tests can show the device rejects them."""
import numpy as np

TWISTS = np.array([[0.22, 0.0], [0.22, 2.0], [0.22, -2.0]])


def forward(p, x):
    """p: dict w1 b1 w2 b2 w3 b3 (float64, nn.Linear layout).  -> (q, h1, h2)."""
    h1 = np.maximum(x @ p["w1"].T + p["b1"], 0.0)
    h2 = np.maximum(h1 @ p["w2"].T + p["b2"], 0.0)
    return h2 @ p["w3"].T + p["b3"], h1, h2


def grads(p, x, dq):
    """Gradients of sum(dq * q) w.r.t. every parameter (dq already holds the loss's 1 / n factors)."""
    q, h1, h2 = forward(p, x)
    dz2 = (dq @ p["w3"]) * (h2 > 0)
    dz1 = (dz2 @ p["w2"]) * (h1 > 0)
    return dict(w3=dq.T @ h2, b3=dq.sum(0), w2=dz2.T @ h1, b2=dz2.sum(0), w1=dz1.T @ x, b1=dz1.sum(0))


def x_batch(s, a, r, s2, d, q_s, q_next, gamma):
    """deepq.py:228-262: X_batch, Y_batch in the reference's row order, and each row's source (m, or B + m for a final s2 row)."""
    B = s.shape[0]
    X, Y, src = [], [], []
    for m in range(B):
        t = r[m] if d[m] else r[m] + gamma * np.max(q_next[m])
        y = q_s[m].copy()
        y[int(a[m])] = t
        X.append(s[m]); Y.append(y); src.append(m)
        if d[m]:
            X.append(s2[m]); Y.append(np.full(q_s.shape[1], r[m])); src.append(B + m)
    return np.array(X), np.array(Y), np.array(src)


def rmsprop(p, acc, g, lr, rho, eps, eps_in_sqrt=False):
    out, acc2 = {}, {}
    for k in p:
        a = rho * acc[k] + (1.0 - rho) * g[k] ** 2
        acc2[k] = a
        out[k] = p[k] - lr * g[k] / (np.sqrt(a + eps) if eps_in_sqrt else np.sqrt(a) + eps)
    return out, acc2


def update(p, p_t, acc, batch, perm, gamma, lr, rho, eps, use_target, variant=None):
    """One learnOnMiniBatch + fit.  batch = (s, a, r, s2, d) with s / s2 already cut to the network's inputs.  variant: None (the
    reference), "chosen_only" (chunk 2's gradient on the chosen column only), "skip_chunk2", "phantom" (a zero-gradient second
    step when F = 0), "eps_in_sqrt", "target_early" (Q' = the target net before the first copy).
    -> (params, accumulators, dict(X, Y, src, g1, g2, loss1, loss2))."""
    s, a, r, s2, d = batch
    B = s.shape[0]
    ut = use_target or variant == "target_early"
    q_s = forward(p, s)[0]
    q_next = forward(p_t if ut else p, s2)[0]
    X, Y, src = x_batch(s, a, r, s2, d, q_s, q_next, gamma)
    n = X.shape[0]
    perm = np.asarray(perm)
    info = dict(X=X, Y=Y, src=src)
    ein = variant == "eps_in_sqrt"
    chunks = [perm[:B], perm[B:]]
    for c, idx in enumerate(chunks):
        if c == 1 and (len(idx) == 0 and variant != "phantom" or variant == "skip_chunk2"):
            break
        q = forward(p, X[idx])[0] if len(idx) else np.zeros((0, Y.shape[1]))
        dq = 2.0 * (q - Y[idx]) / (Y.shape[1] * max(len(idx), 1))
        if c == 1 and variant == "chosen_only":
            mask = np.zeros_like(dq)
            for i, xr in enumerate(idx):
                m = src[xr]
                if m < B:
                    mask[i, int(a[m])] = 1.0
            dq = dq * mask
        g = grads(p, X[idx], dq) if len(idx) else {k: np.zeros_like(v) for k, v in p.items()}
        info["g%d" % (c + 1)] = g
        info["loss%d" % (c + 1)] = float(np.mean((q - Y[idx]) ** 2)) if len(idx) else 0.0
        p, acc = rmsprop(p, acc, g, lr, rho, eps, ein)
    return p, acc, info


def epsilon_draw(seed, counter, row):
    """cn_dqn_act's draws for (seed, counter, row): (u in [0, 1) with 53 bits, uniform index in {0, 1, 2})."""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    h = mix(mix(seed ^ mix(counter ^ 0x2545F4914F6CDD1D)) ^ (row & 0xFFFFFFFF))
    u = (h >> 11) / 9007199254740992.0
    h2 = mix(h ^ 0x9E3779B97F4A7C15)
    return u, ((h2 >> 32) * 3) >> 32
