"""A float64 restatement of the reference's DQN update (deepq.py:219-266, memory.py:22-28, Keras fit / mse / RMSprop) and action
selection, for the parity tests.  Variants that are NOT the reference are switches, so the tests can show the device rejects them.

The second half states what the fused kernels (csrc/crowdnav_dqn.hip) add to that: the plan dqn_prep_kernel makes (the drawn
Fisher-Yates shuffle, the replay row of every sample, the chunk marks and the flags), and one update as a td3_f64._Pass evaluation
on the 2B stacked rows [s; s2] the device works on, so that td3_f64.propagated_bounds gives every quantity of it -- Q, Y, the six
gradients of either chunk, both losses, the stepped weights and accumulators -- a float32 rounding bound (LAMBDA x the propagated
RMS).  The shuffle, the replay row and cn_dqn_act's epsilon draw are three uses of ONE hash, mix64(mix64(seed ^ mix64(c')) ^ row),
that differ only in the salt folded into the counter: c' = c for the replay row, c ^ 0x3c6ef372fe94f82b for the shuffle,
c ^ 0x2545f4914f6cdd1d for epsilon."""
import numpy as np
import torch

import sampling_f64 as S
import td3_f64 as R
from actor_f64 import MASK64, noise_key
from adam_series import pow2_at_least             # noqa: F401 (dqn_f64.pow2_at_least to its tests)

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


# ---- what dqn_prep_kernel plans: exact integers ------------------------------------------------------------------------------
NAMES = R.NAMES
SHUFFLE_XOR = 0x3C6EF372FE94F82B
SHUFFLE_VARIANTS = ("ascending", "counter+1")
# wrong statements of the update the tests must be able to tell from the device (update_pass's `variant`)
VARIANTS = ("chosen_only", "skip_chunk2", "eps_in_sqrt", "target_early", "mse_n", "chunk2_over_B", "extra_from_q", "max_online")


def draw_shuffle(seed, counter, n, variant=None):
    """The permutation of the n = B + F X_batch rows the device draws for update `counter` when no perm is given: Fisher-Yates
    with the draws j_i = mix(mix(seed ^ mix(counter ^ 0x3c6ef372fe94f82b)) ^ i) % (i + 1) and the swaps (i, j_i) from i = n - 1
    down to 1.  variant: "ascending" (the swaps from i = 1 up), "counter+1"."""
    c = int(counter) + (1 if variant == "counter+1" else 0)
    i = np.arange(n, dtype=np.int64)
    j = (noise_key(seed, (c ^ SHUFFLE_XOR) & MASK64, i) % (i + 1).astype(np.uint64)).astype(np.int64)
    perm = i.copy()
    for k in (range(1, n) if variant == "ascending" else range(n - 1, 0, -1)):
        perm[k], perm[j[k]] = perm[j[k]], perm[k]
    return perm


def replay_row(seed, counter, m, size):
    """The ring row of batch row(s) m of update `counter` at live size `size`: mix(mix(seed ^ mix(counter)) ^ m) % max(size, 1) --
    the rule of the TD3 / DDPG replay path (sampling_f64.indices), unsalted."""
    return S.indices(seed, counter, None, size, rows=np.atleast_1d(m))


def plan(d, counter, target_every, seed=0, perm=None, live=True, variant=None):
    """The plan of one update: X_batch's row order (sample m's s row m, then its s2 row B + m when final), the shuffle (given or
    drawn), chunk[g] of every stacked row (1: among the first B shuffled rows, 2: the F after them, 0: not in X_batch; all 0 while
    the replay waits for learn_start) and flags 0-4 (live, chunk 2 runs, F, Q' = the target net, copy after this update)."""
    fin = np.asarray(d) != 0
    B = len(fin)
    order = []
    for m in range(B):
        order.append(m)
        if fin[m]:
            order.append(B + m)
    order = np.array(order, dtype=np.int64)
    n = len(order)
    F = n - B
    perm = draw_shuffle(seed, counter, n, variant) if perm is None else np.asarray(perm, dtype=np.int64)
    chunk = np.zeros(2 * B, dtype=np.int32)
    if live:
        chunk[order[perm[:B]]] = 1
        chunk[order[perm[B:]]] = 2
    flags = np.array([live, live and F > 0, F, counter >= target_every, live and (counter + 1) % target_every == 0], dtype=np.int32)
    return dict(chunk=chunk, flags=flags, perm=perm, order=order, F=F)


# ---- one update on the stacked rows, as a td3_f64._Pass evaluation -------------------------------------------------------------
def new_params(obs_dim, hidden, gen, device="cpu"):
    """nn.Linear's default initialisation (weights AND biases uniform +-1 / sqrt(fan_in)) of the three layers, float32."""
    def lin(i, o):
        k = 1.0 / np.sqrt(i)
        return [((torch.rand(sh, generator=gen, dtype=torch.float64) * 2 - 1) * k).float().to(device) for sh in ((o, i), (o,))]
    return dict(zip(NAMES, lin(obs_dim, hidden) + lin(hidden, hidden) + lin(hidden, 3)))


def to64(p):
    return {k: v.detach().double() for k, v in p.items()}


def acc0(p):
    """RMSprop's accumulators at create: zeros (float64)."""
    return {k: torch.zeros_like(v, dtype=torch.float64) for k, v in p.items()}


def within(ratios):
    """Every error / bound ratio is <= 1 (a NaN ratio -- a NaN from the device -- is not)."""
    return all(r <= 1.0 for r in ratios.values())


def hyper(gamma, lr, rho, eps):
    """The optimiser's constants as the float32 values the kernel receives (1 - rho is exact in float32 for rho in [0.5, 1])."""
    f = np.float32
    return dict(gamma=float(f(gamma)), lr=float(f(lr)), rho=float(f(rho)), omr=float(f(1) - f(rho)), eps=float(f(eps)))


def chain_length(obs_dim, hidden):
    """Roundings on the longest chain to a pre-activation (D + 1 to the first layer's, H + 1 more to the second's) and 64 spare for
    the partial-sum tiles: the N of the strict ReLU-margin bound N u (|x||W| + |b|)."""
    return obs_dim + hidden + 2 + 64


def plant_dead_units(p, hidden):
    """td3_f64.plant_dead_units on the one network: unit 1 of layer 1 and unit hidden - 2 of layer 2 -> (u1, u2) or None."""
    return R.plant_dead_units({"q": p}, hidden, nets=("q",)).get("q")


def dead_slices(p, dead):
    """The slices of the six tensors a dead pair of units owns (in and out): every one must come back bit for bit."""
    return [] if dead is None else R.dead_slices(p, dead)


def establish_margins(p, X2, N, pt=None):
    """td3_f64's bias placement for the one network on ALL 2B stacked rows [s; s2] (and the target network on the s2 rows): no
    pre-activation of a live unit lies within N u (|x||W| + |b|) of zero, so every ReLU mask is the same in float32 and float64."""
    B = X2.shape[0] // 2
    for q, x in ((p, X2),) + (((pt, X2[B:]),) if pt is not None else ()):
        x = x.double()
        R._layer_margins(q["w1"], q["b1"], [x], [x.abs()], N)
        f = R._mlp(to64(q), x, x.abs())
        R._layer_margins(q["w2"], q["b2"], [f["h1"]], [f["m_h1"]], N)


def margin_ratio(p, x, N):
    """min over live units and rows of |pre-activation| / (N u magnitude): >= 1 means no mask is ambiguous."""
    q, x = to64(p), x.double()
    f = R._mlp(q, x, x.abs())
    worst = float("inf")
    for z, m, w, b in ((f["z1"], f["m_z1"], q["w1"], q["b1"]), (f["z2"], f["m_z2"], q["w2"], q["b2"])):
        r_ = (z.abs() / (N * R.U * m))[:, ~R._is_dead(w, b)]
        if r_.numel():
            worst = min(worst, float(r_.min()))
    return worst


def act_pass(ps, p, x):
    return {"q": ps.mlp(p, x, "q")["out"]}


def _targets(ps, p, pt, use_target, X2, a, r, d, gamma, variant, tag, zs):
    """Q on the 2B rows and Y (deepq.py:240-262): rows < B: Q(s) with the chosen column replaced by r or r + gamma max Q'(s2);
    rows >= B: [r, r, r].  The unchosen columns of Y ARE the device's q, so their error is exactly zero."""
    B = a.shape[0]
    f = ps.mlp(p, X2, tag + "q")
    q = f["out"]
    zs.update({tag + "q.1": f["z1"], tag + "q.2": f["z2"]})
    ut = (use_target and variant != "max_online") or variant == "target_early"
    qn = q[B:]
    if ut:
        ft = ps.mlp(pt, X2[B:], tag + "qt")
        qn = ft["out"]
        zs.update({tag + "qt.1": ft["z1"], tag + "qt.2": ft["z2"]})
    t = torch.where(d != 0, r, ps.ew(r + ps.ew(gamma * qn.max(1).values)))
    extra = q[B:] if variant == "extra_from_q" else r[:, None].expand(B, 3)
    return f, torch.cat([q[:B].scatter(1, a[:, None], t[:, None]), extra], 0)


def _chunk(ps, p, X2, f, Y, mark, which, n, a, variant):
    """dq = 2 (q - Y) / (3 n) on the rows marked `which` (0 elsewhere), the six gradients over all 2B rows, the chunk's loss."""
    B = a.shape[0]
    inn = (mark == which).to(Y.dtype)[:, None]
    e = ps.ew(f["out"] - Y) * inn
    dq = ps.ew(2.0 * e / ((1.0 if variant == "mse_n" else 3.0) * n), 2.0)
    if which == 2 and variant == "chosen_only":
        dq = dq * torch.cat([torch.zeros_like(dq[:B]).scatter(1, a[:, None], 1.0), torch.zeros_like(dq[B:])], 0)
    g, _ = ps.backward(p, X2, f, dq)
    ones = torch.ones((e.numel(), 1), dtype=e.dtype, device=e.device)
    return g, ps.ew(ps.mm((e * e).reshape(1, -1), ones)[0, 0] / (3.0 * n))


def _step(ps, p, acc, g, hp, variant):
    """Keras 2's RMSprop: a = rho a + (1 - rho) g^2, w -= lr g / (sqrt(a) + eps)."""
    p2, acc2 = {}, {}
    for k in NAMES:
        a_ = ps.ew(hp["rho"] * acc[k] + hp["omr"] * ps.ew(g[k] * g[k]), 2.0)
        den = ps.ew(torch.sqrt(a_ + hp["eps"])) if variant == "eps_in_sqrt" else ps.ew(ps.ew(torch.sqrt(a_)) + hp["eps"])
        acc2[k] = a_
        p2[k] = ps.ew(p[k] - ps.ew(hp["lr"] * g[k] / den, 2.0))
    return p2, acc2


def update_pass(ps, p, pt, acc, batch, mark, hp, use_target, variant=None, only=None, tag=""):
    """One cn_dqn_update.  batch = (s, a int64, r, s2, d) float64 with s / s2 cut to the inputs; mark = plan()["chunk"] as a tensor.
    only=2: chunk 1's step is known to be null (its error is exactly zero on the device), chunk 2 runs at the given weights.
    variant "phantom": a zero-gradient second step when F = 0.  -> flat {"q", "Y", "loss1", "loss2", "g1.w1".., "p1.w1".., "g2..",
    "p2.w1".. (the final weights), "acc.w1".. (the final accumulators), "z:<mask key>" (the pre-activations of every forward; `tag`
    keeps the mask keys of consecutive updates apart)}."""
    s, a, r, s2, d = batch
    B = a.shape[0]
    X2 = torch.cat([s, s2], 0)
    F = int((mark == 2).sum())
    zs = {}
    f, Y = _targets(ps, p, pt, use_target, X2, a, r, d, hp["gamma"], variant, tag, zs)
    zero = torch.zeros((), dtype=Y.dtype, device=Y.device)
    out = {"q": f["out"], "Y": Y, "loss1": zero, "loss2": zero}
    if only != 2:
        g1, out["loss1"] = _chunk(ps, p, X2, f, Y, mark, 1, B, a, variant)
        p, acc = _step(ps, p, acc, g1, hp, variant)
        out.update({"g1." + k: g1[k] for k in NAMES})
        out.update({"p1." + k: p[k] for k in NAMES})
    if (F > 0 and variant != "skip_chunk2") or variant == "phantom":
        f2 = f if only == 2 else ps.mlp(p, X2, tag + "q2")
        n2 = B if variant == "chunk2_over_B" else max(F, 1)
        g2, out["loss2"] = _chunk(ps, p, X2, f2, Y, mark, 2, n2, a, variant)
        p, acc = _step(ps, p, acc, g2, hp, variant)
        out.update({"g2." + k: g2[k] for k in NAMES})
        if only != 2:
            zs.update({tag + "q2.1": f2["z1"], tag + "q2.2": f2["z2"]})
    out.update({"p2." + k: p[k] for k in NAMES})
    out.update({"acc." + k: acc[k] for k in NAMES})
    out.update({"z:" + k: v for k, v in zs.items()})
    return out


def part(out, prefix):
    return {k: out[prefix + "." + k] for k in NAMES}


class _Held(R._Pass):
    """Exact arithmetic with the ReLU masks GIVEN (one of them flipped: what an ambiguous mask would do on the device)."""

    def mask(self, key, z):
        return self.masks[key]


def bounded(run, samples=R.SAMPLES, max_flips=256):
    """(exact float64 values, bounds, number of ambiguous masks) of a pass.  The bounds are td3_f64.propagated_bounds' LAMBDA x
    propagated RMS.  The first forward of a handle has its masks fixed by construction (establish_margins); every later forward
    runs on weights that carry the steps' own float32 error, and where a pre-activation of such a forward lies within its bound of
    zero the device may take either mask.  Each such entry is flipped alone in an exact run and the change of every quantity is
    ADDED to its bound.  ASSUMPTION, not a derivation: the flips' effects add.  That holds to first order (each flip adds its own
    rank-one term to a gradient); how two flips interact -- one flip moving a later pre-activation across zero, or two flips on
    one row -- is second order and is NOT bounded here.  Nothing of it is looked up from the device."""
    exact, bound = R.propagated_bounds(run, samples=samples)
    first = R._Pass()
    run(first)
    amb = []
    for k in exact:
        if k.startswith("z:"):
            amb += [(k[2:], tuple(i)) for i in ((exact[k].abs() < bound[k]) & (bound[k] > 0)).nonzero().tolist()]
    assert len(amb) <= max_flips, len(amb)
    for mk, idx in amb:
        masks = dict(first.masks)
        masks[mk] = masks[mk].clone()
        masks[mk][idx] = 1 - masks[mk][idx]
        alt = run(_Held(None, masks))
        for k in bound:
            if not k.startswith("z:"):
                bound[k] = bound[k] + (alt[k] - exact[k]).abs()
    return exact, bound, len(amb)


def series_pass(ps, p, pt, hp, target_every, batches, marks, variant=None):
    """Consecutive updates of one handle (weights, accumulators, the target net and the counter carried from one to the next, so
    a bound on update u holds the errors of all before it).  Keys "u<u>.<update_pass key>" and "u<u>.t.w1".. (the target net)."""
    acc = {k: torch.zeros_like(v) for k, v in p.items()}
    out = {}
    for u, (batch, mark) in enumerate(zip(batches, marks)):
        o = update_pass(ps, p, pt, acc, batch, mark, hp, u >= target_every, variant, tag="u%d." % u)
        p, acc = part(o, "p2"), part(o, "acc")
        if (u + 1) % target_every == 0:
            pt = p
        out.update({(k if k.startswith("z:") else "u%d.%s" % (u, k)): v for k, v in o.items()})
        out.update({"u%d.t.%s" % (u, k): pt[k] for k in NAMES})
    return out


# ---- the GPU tests' plan (tests/test_gpu_dqn_f64.py), here so that the CPU tests can run the same cases without a device -------
ACT_HIDDEN = (1, 15, 16, 17, 31, 32, 33, 300, 479, 480)
ACT_D = (1, 3, 15, 16, 17, 127, 128, 129, 361)
ACT_N = (1, 15, 16, 17, 65541)
PRODUCT = (361, 363, 300, 64)                                   # (D, ld, H, B)
RAGGED = (33, 35, 33, 17)
UPDATE_SHAPES = ([PRODUCT] + [(45, 47, h, 40) for h in (1, 3, 15, 16, 17, 31, 32, 33, 257)]
                 + [(d, d + (3 if d % 2 else 0), 40, 24) for d in (1, 14, 15, 16, 30, 31, 32)]
                 + [(20, 20, 48, b) for b in (1, 3, 33, 127, 129)] + [(361, 363, 300, 4096), (361, 363, 4096, 64)])
DISCRIMINATE = (PRODUCT, RAGGED)
SERIES_F = (3, 0, 0, None, 0, 1, 0, 0)                           # None = B: every sample final
LR_RECOVER = 1024.0                                              # rho = 0: w' = w - lr g / (|g| + eps), inverted per element


def make_case(shape, n_final=0, seed=0, device="cpu", margins=True, scale3=1.0):
    """Weights (dead units planted, ReLU margins on all 2B stacked rows; a target net that differs), and a float32 batch
    (s, a int32, r, s2, d) with NaN in the padding columns of s and s2.  -> (p, pt, batch, dead, N)."""
    D, ld, H, B = shape
    g = torch.Generator().manual_seed(seed + 1000 * H + 10 * B + D)
    p, pt = new_params(D, H, g), new_params(D, H, g)
    p["w3"] *= scale3
    s, s2 = torch.full((B, ld), float("nan")), torch.full((B, ld), float("nan"))
    s[:, :D] = torch.randn((B, D), generator=g) * 0.5
    s2[:, :D] = torch.randn((B, D), generator=g) * 0.5
    a = torch.randint(0, 3, (B,), generator=g).to(torch.int32)
    r = (2 + 0.5 * torch.randn(B, generator=g)).float()
    d = torch.zeros(B)
    d[torch.randperm(B, generator=g)[:n_final]] = 1.0
    dead = plant_dead_units(p, H) if margins else None
    N = chain_length(D, H)
    if margins:
        establish_margins(p, torch.cat([s[:, :D], s2[:, :D]], 0), N, pt)
    mv = lambda t: t.to(device).contiguous()
    return ({k: mv(v) for k, v in p.items()}, {k: mv(v) for k, v in pt.items()}, tuple(mv(t) for t in (s, a, r, s2, d)), dead, N)


def batch64(batch, D):
    s, a, r, s2, d = batch
    return (s[:, :D].double(), a.long(), r.double(), s2[:, :D].double(), d.double())


def stacked(batch, D):
    return torch.cat([batch[0][:, :D], batch[3][:, :D]], 0)


def final_perm(B, rng=None):
    """Every sample final: X_batch is s_0, s2_0, s_1, s2_1, ...; this shuffle puts the B s rows in chunk 1 and the B extra rows
    in chunk 2 (each half in a random order when rng is given)."""
    first, second = np.arange(B) * 2, np.arange(B) * 2 + 1
    if rng is not None:
        first, second = rng.permutation(first), rng.permutation(second)
    return np.concatenate([first, second])


def act_case(hidden, obs_dim, ld, n, device="cpu"):
    """cn_dqn_act's inputs: weights and n observation rows, NaN in the ld - obs_dim padding columns (the same values whatever ld)."""
    g = torch.Generator().manual_seed(hidden * 1000 + obs_dim)
    p = new_params(obs_dim, hidden, g)
    x = torch.full((n, ld), float("nan"))
    x[:, :obs_dim] = torch.randn((n, obs_dim), generator=g) * 0.5
    return {k: v.to(device).contiguous() for k, v in p.items()}, x.to(device).contiguous()


def unclear_rows(q, bound):
    """Rows whose float64 best and second-best Q lie within twice the row's largest bound: their argmax is not compared."""
    top = q.topk(2, 1).values
    return (top[:, 0] - top[:, 1]) <= 2.0 * bound.max(1).values
