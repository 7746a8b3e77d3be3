"""TEST INFRASTRUCTURE.  A float64 restatement of what cn_sac_update computes per row (sac.py:253-272 of the reference): the
heads, the sample, the double squash, log_prob, the four network outputs, the three losses and the per-row loss gradients, with
the gradients BY FORMULA (rows()), and the whole update -- those and every weight gradient of Q, V and the actor -- as a
td3_f64._Pass evaluation (run()) whose perturbed runs give the error bounds (reference()).  tests/test_sac_f64_helpers.py holds
both to torch.autograd on the reference's loss expressions.

Parameters are dicts {net: {name: tensor}} like tests/td3_f64.py's: actor = w1, b1, w2, b2, mean_w, mean_b, ls_w, ls_b;
q, v, v_t = td3_f64.NAMES.  `variant` restates the update WRONGLY in one named way (the discrimination tests)."""
import math

import torch

import td3_f64 as R
from td3_f64 import NAMES                      # ("w1", "b1", "w2", "b2", "w3", "b3")

ACTOR_NAMES = ("w1", "b1", "w2", "b2", "mean_w", "mean_b", "ls_w", "ls_b")
CFG = dict(gamma=0.99, max_v=0.22, max_w=2.0, ls_min=-20.0, ls_max=2.0, mean_lambda=1e-3, std_lambda=1e-3, z_lambda=0.0, logp_eps=1e-6)
KEYS = ("a_new", "dl", "dq", "dv", "loss")      # what a comparison looks at
VARIANTS = ("rsample", "single_squash", "first_sample", "unclamped_regulariser", "scaled_gradient")
EPS32 = 2.0 ** -24
Z_STEP_MAX = 2.0                                # make_case: |eps| std <= this (|eps| <= 3 before)
EPS0_BELOW = -4.0                               # make_case: eps = 0 where the raw log_std is below this


def new_params(obs_dim, hidden, hidden_v, gen, head_scale=1.0, device="cpu", dtype=torch.float32):
    """nn.Linear-like draws; the log_std head scaled by head_scale so that rows fall below, inside and above the clamp."""
    def lin(o, i, s=None):
        k = 1.0 / math.sqrt(i) if s is None else s
        return (torch.rand((o, i), generator=gen) * 2 - 1) * k, (torch.rand(o, generator=gen) * 2 - 1) * k
    P = {}
    w1, b1 = lin(hidden, obs_dim); w2, b2 = lin(hidden, hidden); mw, mb = lin(2, hidden, 0.05); lw, lb = lin(2, hidden, 0.05 * head_scale)
    P["actor"] = dict(zip(ACTOR_NAMES, (w1, b1, w2, b2, mw, mb, lw, lb)))
    for net, i, h in (("q", obs_dim + 2, hidden), ("v", obs_dim, hidden_v), ("v_t", obs_dim, hidden_v)):
        w1, b1 = lin(h, i); w2, b2 = lin(h, h); w3, b3 = lin(1, h)
        P[net] = dict(zip(NAMES, (w1, b1, w2, b2, w3, b3)))
    return {n: {k: v.to(dtype).to(device).contiguous() for k, v in p.items()} for n, p in P.items()}


def to64(P):
    return {n: {k: v.detach().double().cpu() for k, v in p.items()} for n, p in P.items()}


def mlp(p, x):
    h1 = torch.relu(x @ p["w1"].T + p["b1"])
    h2 = torch.relu(h1 @ p["w2"].T + p["b2"])
    return (h2 @ p["w3"].T + p["b3"]).reshape(-1), h1, h2


def trunk(p, s):
    h1 = torch.relu(s @ p["w1"].T + p["b1"])
    h2 = torch.relu(h1 @ p["w2"].T + p["b2"])
    return h2 @ p["mean_w"].T + p["mean_b"], h2 @ p["ls_w"].T + p["ls_b"], h1, h2


def rows(P, batch, eps, cfg=CFG, variant=None, eps_first=None):
    """Everything per row, float64.  P, batch, eps: float64 CPU tensors.  -> dict."""
    s, a, r, s2, d = batch
    B = s.shape[0]
    c = cfg
    mean, raw, _, _ = trunk(P["actor"], s)
    ls = raw.clamp(c["ls_min"], c["ls_max"])
    sd = ls.exp()
    e = eps_first if variant == "first_sample" else eps
    z = e * sd + mean
    t = torch.tanh(z)
    logp = (-((z - mean) ** 2) / (2 * sd ** 2) - sd.log() - 0.5 * math.log(2 * math.pi) - torch.log(1 - t ** 2 + c["logp_eps"])).sum(1)
    if variant == "single_squash":
        a_new = torch.stack([t[:, 0] * c["max_v"], t[:, 1] * c["max_w"]], 1)
    else:
        a_new = torch.stack([torch.sigmoid(t[:, 0]) * c["max_v"], torch.tanh(t[:, 1]) * c["max_w"]], 1)
    q, _, _ = mlp(P["q"], torch.cat([s, a], 1))
    v, _, _ = mlp(P["v"], s)
    vt, _, _ = mlp(P["v_t"], s2)
    qn, _, _ = mlp(P["q"], torch.cat([s, a_new], 1))
    y = r + (1 - d) * c["gamma"] * vt
    coef = (logp - (qn - v)) / B
    dq = 2 * (q - y) / B
    dv = 2 * (v - (qn - logp)) / B
    inside = ((raw >= c["ls_min"]) & (raw <= c["ls_max"])).double()
    e_ = (z - mean) / sd
    g_mean = coef[:, None] * e_ / sd + c["mean_lambda"] * mean / B
    g_ls = coef[:, None] * (e_ ** 2 - 1) * inside
    if variant == "rsample":
        # z = mean + std eps carries a gradient: Normal.log_prob's terms in z cancel, -log(1 - tanh^2 + eps) gains one through z
        dz = 2 * t * (1 - t ** 2) / (1 - t ** 2 + c["logp_eps"])
        g_mean = coef[:, None] * dz + c["mean_lambda"] * mean / B
        g_ls = coef[:, None] * (-1 + dz * e * sd) * inside
    if variant == "unclamped_regulariser":
        g_ls = g_ls + c["std_lambda"] * raw / B
    else:
        g_ls = g_ls + c["std_lambda"] * ls / B * inside
    dl = torch.cat([g_mean, g_ls], 1)
    if variant == "scaled_gradient":
        dl, dq, dv = dl * (1 + 1e-3), dq * (1 + 1e-3), dv * (1 + 1e-3)
    loss = torch.stack([((q - y) ** 2).mean(), ((v - (qn - logp)) ** 2).mean(),
                        (logp * (logp - (qn - v))).mean() + c["mean_lambda"] * (mean ** 2).mean() + c["std_lambda"] * (ls ** 2).mean()
                        + c["z_lambda"] * (z ** 2).sum(1).mean()])
    return dict(mean=mean, log_std=ls, raw=raw, z=z, logp=logp, a_new=a_new, q=q, v=v, vt=vt, qn=qn, y=y, dq=dq, dv=dv, dl=dl, loss=loss,
                inside=inside, sd=sd)


def _lin(ps, h, w, b):
    ones = torch.ones((h.shape[0], 1), dtype=h.dtype, device=h.device)
    return ps.mm(torch.cat([h, ones], 1), torch.cat([w, b[:, None]], 1).T)


def run(ps, P, batch, eps, cfg=CFG, variant=None, eps_first=None):
    """One update as a td3_f64._Pass evaluation, operation by operation as sac_head_kernel / sac_loss_kernel and the GEMM jobs
    compute it (exact with _Pass(), or with every rounding perturbed: td3_f64.propagated_bounds).  -> the per-row quantities
    of KEYS and the weight gradients of Q, V and the actor as (net, name).  The ReLU masks and the clamp classes are those of
    the exact run (the margins guarantee that float32 decides them alike)."""
    s, a, r, s2, d = batch
    B, c, pa = s.shape[0], cfg, P["actor"]
    z1 = _lin(ps, s, pa["w1"], pa["b1"]); m1 = ps.mask("actor.1", z1); h1 = z1 * m1
    z2 = _lin(ps, h1, pa["w2"], pa["b2"]); m2 = ps.mask("actor.2", z2); h2 = z2 * m2
    mean, raw = _lin(ps, h2, pa["mean_w"], pa["mean_b"]), _lin(ps, h2, pa["ls_w"], pa["ls_b"])
    if ps.gen is None:
        ps.masks["lo"], ps.masks["hi"] = (raw < c["ls_min"]).to(raw.dtype), (raw > c["ls_max"]).to(raw.dtype)
    lo, hi = ps.masks["lo"], ps.masks["hi"]
    inside = 1 - lo - hi
    ls = raw * inside + lo * c["ls_min"] + hi * c["ls_max"]
    sd = ps.ew(ls.exp(), 4.0)
    e = eps_first if variant == "first_sample" else eps
    step = ps.ew(e * sd)
    z = ps._noise(step + mean, R.U * (step + mean).abs() * (step != 0))          # eps = 0: z = mean exactly
    t = ps.ew(torch.tanh(z), 4.0).clamp(-1.0, 1.0)                            # tanhf never leaves [-1, 1]
    dz, var = ps.ew(z - mean), ps.ew(sd * sd)
    om = ps.ew(ps.ew(1 - ps.ew(t * t)) + c["logp_eps"])                       # 1 - t^2 cancels: t^2's rounding lands on it absolutely
    terms = torch.stack([-ps.ew(ps.ew(dz * dz) / (2 * var), 2.0), -ps.ew(sd.log(), 4.0), torch.full_like(z, -0.5 * math.log(2 * math.pi)),
                         -ps.ew(om.log(), 4.0)], 2)
    logp = ps._noise(terms.sum((1, 2)), 8 * R.U * terms.abs().sum((1, 2)))
    if variant == "single_squash":
        a_new = ps.ew(torch.stack([t[:, 0] * c["max_v"], t[:, 1] * c["max_w"]], 1))
    else:
        a_new = ps.ew(torch.stack([torch.sigmoid(t[:, 0]) * c["max_v"], torch.tanh(t[:, 1]) * c["max_w"]], 1), 4.0)
    xq, xn = torch.cat([s, a], 1), torch.cat([s, a_new], 1)
    fq, fv = ps.mlp(P["q"], xq, "q"), ps.mlp(P["v"], s, "v")
    q, v = fq["out"][:, 0], fv["out"][:, 0]
    vt, qn = ps.mlp(P["v_t"], s2, "v_t")["out"][:, 0], ps.mlp(P["q"], xn, "qn")["out"][:, 0]
    y = ps.ew(r + ps.ew((1 - d) * c["gamma"] * vt, 2.0))
    cdet = ps.ew(logp - ps.ew(qn - v))
    coef = ps.ew(cdet / B)[:, None]
    eq, ev = ps.ew(q - y), ps.ew(v - ps.ew(qn - logp))
    dq, dv = ps.ew(2.0 * eq / B, 2.0), ps.ew(2.0 * ev / B, 2.0)
    q2 = ps.ew(ps.ew(dz * dz) / var)
    if variant == "rsample":             # z carries a gradient: Normal.log_prob's terms in z cancel, -log(1 - tanh^2 + eps) gains one
        dzt = 2 * t * (1 - t ** 2) / (1 - t ** 2 + c["logp_eps"])
        gm = coef * dzt + c["mean_lambda"] * mean / B
        gs = inside * (coef * (-1 + dzt * e * sd) + c["std_lambda"] * ls / B)
    else:
        gm = ps.ew(ps.ew(coef * dz / var, 2.0) + ps.ew(c["mean_lambda"] * mean / B, 2.0))
        gs = inside * ps.ew(ps.ew(coef * ps.ew(q2 - 1)) + ps.ew(c["std_lambda"] * ls / B, 2.0))
    if variant == "unclamped_regulariser":
        gs = inside * ps.ew(coef * ps.ew(q2 - 1)) + c["std_lambda"] * raw / B
    dl = torch.cat([gm, gs], 1)
    out = dict(mean=mean, raw=raw, log_std=ls, z=z, logp=logp, qn=qn, a_new=a_new, dq=dq, dv=dv, dl=dl)
    for net, x, f, dout in (("q", xq, fq, dq), ("v", s, fv, dv)):
        g, _ = ps.backward(P[net], x, f, dout[:, None])
        out.update({(net, k_): g_ for k_, g_ in g.items()})
    g = {}
    g["mean_w"], g["mean_b"] = ps.wgrad(gm, h2)
    g["ls_w"], g["ls_b"] = ps.wgrad(gs, h2)
    dz2 = ps.mm(dl, torch.cat([pa["mean_w"], pa["ls_w"]], 0)) * m2
    g["w2"], g["b2"] = ps.wgrad(dz2, h1)
    dz1 = ps.mm(dz2, pa["w2"]) * m1
    g["w1"], g["b1"] = ps.wgrad(dz1, s)
    out.update({("actor", k_): g_ for k_, g_ in g.items()})
    ones = torch.ones((1, B), dtype=s.dtype, device=s.device)
    tot = lambda x: ps.mm(ones, x.reshape(B, -1)).sum()
    out["loss"] = torch.stack([ps.ew(tot(ps.ew(eq * eq)) / B), ps.ew(tot(ps.ew(ev * ev)) / B),
                               ps.ew(ps.ew(tot(ps.ew(logp * cdet)) / B) + ps.ew(c["mean_lambda"] * tot(ps.ew(mean * mean)) / (2 * B), 2.0)
                                     + ps.ew(c["std_lambda"] * tot(ps.ew(ls * ls)) / (2 * B), 2.0) + ps.ew(c["z_lambda"] * tot(ps.ew(z * z)) / B, 2.0), 2.0)])
    return out


def reference(P, batch, eps, cfg=CFG, variant=None, eps_first=None):
    """(float64 values, bounds) of everything run() returns: the bounds are td3_f64.propagated_bounds' LAMBDA x the RMS change over
    perturbed runs -- they follow the float32 error of each element (an exact zero has bound zero), not its worst case."""
    return R.propagated_bounds(lambda ps: run(ps, P, batch, eps, cfg, variant, eps_first))


GRADS = tuple(("q", k) for k in NAMES) + tuple(("v", k) for k in NAMES) + tuple(("actor", k) for k in ACTOR_NAMES)


def clamp_chain(obs_dim, hidden):
    """Roundings on the way to a raw log_std: the three dot products of the actor's forward pass (each with its bias) and 8 spare
    for the cross-wavefront sums -- the strict count for this quantity; chain_length() counts the whole update's longest chain."""
    return obs_dim + 2 * hidden + 11


def clamp_margin(P, batch, chain):
    """min over the [B][2] raw log_std of |raw - edge| / (chain EPS32 x magnitude): > 1 means float32, in any summation order,
    decides every clamp as float64 does."""
    s, p = batch[0], P["actor"]
    a1 = s.abs() @ p["w1"].abs().T + p["b1"].abs()
    a2 = a1 @ p["w2"].abs().T + p["b2"].abs()
    raw = trunk(p, s)[1]
    ra = a2 @ p["ls_w"].abs().T + p["ls_b"].abs()
    return torch.minimum((raw - CFG["ls_min"]).abs(), (raw - CFG["ls_max"]).abs()) / (chain * EPS32 * ra)


def margins_ok(P, batch, eps, chain, clamp_chain=None):
    """No ReLU mask and no clamp decision may differ between float32 and float64: every pre-activation and every raw log_std keeps
    a distance from its threshold above the forward-error bound of its own dot product."""
    s, a, r, s2, d = batch
    u = chain * EPS32
    ok = True

    def check(p, x):
        nonlocal ok
        z1 = x @ p["w1"].T + p["b1"]; a1 = x.abs() @ p["w1"].abs().T + p["b1"].abs()
        ok = ok and bool((z1.abs() > u * a1).all())
        h1 = torch.relu(z1)
        z2 = h1 @ p["w2"].T + p["b2"]; a2 = a1 @ p["w2"].abs().T + p["b2"].abs()
        ok = ok and bool((z2.abs() > u * a2).all())
    check(P["actor"], s)
    ok = ok and bool((clamp_margin(P, batch, clamp_chain or chain) > 1).all())
    R_ = rows(P, batch, eps)
    check(P["q"], torch.cat([s, a], 1)); check(P["q"], torch.cat([s, R_["a_new"]], 1)); check(P["v"], s); check(P["v_t"], s2)
    return ok


def establish_margins(P, batch, eps, N, which="all"):
    """Shift every hidden unit's bias (td3_f64._layer_margins), network by network in the order the rows depend on each other:
    the actor on s, Q on (s, a) and (s, a_new), V on s, V_t on s2.  Modifies P's float32 tensors in place."""
    s, a, r, s2, d = [x.double() for x in batch]

    def net(name, xs, xms):
        p = P[name]
        R._layer_margins(p["w1"], p["b1"], xs, xms, N)
        p64 = {k: v.double() for k, v in p.items()}
        hs = [(torch.relu(x @ p64["w1"].T + p64["b1"]), xm @ p64["w1"].abs().T + p64["b1"].abs()) for x, xm in zip(xs, xms)]
        R._layer_margins(p["w2"], p["b2"], [h for h, _ in hs], [m for _, m in hs], N)
    if which in ("all", "actor"):
        net("actor", [s], [s.abs()])
    if which == "actor":
        return
    R_ = rows(to64(P), (s, a, r, s2, d), eps.double())
    m_act = torch.full_like(R_["a_new"], 4.0)                  # |a_new| <= 2 and its error's magnitude, generously
    net("q", [torch.cat([s, a], 1), torch.cat([s, R_["a_new"]], 1)], [torch.cat([s, a], 1).abs(), torch.cat([s.abs(), m_act], 1)])
    net("v", [s], [s.abs()])
    net("v_t", [s2], [s2.abs()])


def make_case(obs_dim, hidden, hidden_v, B, seed=0):
    """Parameters (float32 values), a batch and eps such that margins_ok holds -- no ReLU mask and no log_std clamp decision differs
    between float32 and float64 -- with elements clamped at log_std_min, clamped at log_std_max and inside (B >= 3).

    The log_std head: nn.Linear-like small weights plus, per output, one large weight on the second-layer unit whose spread over
    the rows is largest against its magnitude, scaled so that the raw log_std spans 44 units; the bias where the clearance of the
    two clamp edges is largest.  The rounding bound of the raw log_std then is a few hundredths (it scales with that one unit's
    magnitude, not with hidden), and a row that still lies within it of an edge is replaced by a copy of a row that does not
    (a replay batch may hold a transition twice).  eps is zero where the log_std is below EPS0_BELOW = -4 (the clamped elements
    among them): z = eps std + mean rounds to the ulp of mean, so z - mean keeps |eps| std / (2^-24 |mean|) of its digits -- none
    at std = 2e-9 -- and (z - mean) / var, in the reference's own float32 Normal.log_prob as in the kernel, is rounding noise
    that would swamp every other row's share of the actor's gradient.  With eps = 0, z = mean exactly: the mean's gradient
    there is its regulariser's and the log_std's is -coef + its regulariser's (zero where clamped).  Where std is large eps is
    scaled down so that |z - mean| <= Z_STEP_MAX: at std = e^2 an unscaled draw saturates tanh, and log(1 - tanh(z)^2 + 1e-6) in
    float32 then keeps two digits (the rounding of tanh^2 against 1e-6), which would widen every bound that log_prob feeds."""
    chain = R.chain_length(obs_dim, max(hidden, hidden_v), B)
    cc = clamp_chain(obs_dim, hidden)
    for k in range(60):
        g = torch.Generator().manual_seed(1000 * seed + k + 31 * hidden + B)
        P = new_params(obs_dim, hidden, hidden_v, g, head_scale=1.0)
        s = torch.randn((B, obs_dim), generator=g) * 0.5
        a = torch.stack([torch.rand(B, generator=g) * 0.22, torch.rand(B, generator=g) * 4 - 2], 1)
        r = 2 + 0.5 * torch.randn(B, generator=g)
        s2 = torch.randn((B, obs_dim), generator=g) * 0.5
        d = (torch.rand(B, generator=g) < 0.3).float()
        eps = torch.randn((B, 2), generator=g).clamp(-3, 3)
        eps1 = torch.randn((B, 2), generator=g)
        establish_margins(P, (s, a, r, s2, d), eps, chain, which="actor")
        pa = {k_: v.double() for k_, v in P["actor"].items()}
        s64 = s.double()
        h2 = trunk(pa, s64)[3]
        a2 = (s64.abs() @ pa["w1"].abs().T + pa["b1"].abs()) @ pa["w2"].abs().T + pa["b2"].abs()
        spread = h2.max(0).values - h2.min(0).values
        units = torch.argsort(spread / a2.max(0).values, descending=True)[:2].tolist()
        if B < 2 or float(spread[units[0]]) <= 0:
            continue
        for o in range(2):
            j = units[o % len(units)]
            if float(spread[j]) > 0:
                P["actor"]["ls_w"][o, j] = (44.0 if o == 0 else -44.0) / float(spread[j])
        pa = {k_: v.double() for k_, v in P["actor"].items()}
        raw0 = h2 @ pa["ls_w"].T
        ra = a2 @ pa["ls_w"].abs().T + 22.0
        for o in range(2):
            best, best_t = -1.0, 0.0
            for t_ in torch.linspace(-12.0, -6.0, 241).tolist():
                x = raw0[:, o] - raw0[:, o].mean() + t_
                clear = torch.minimum((x - CFG["ls_min"]).abs(), (x - CFG["ls_max"]).abs()) / ra[:, o]
                score = float(clear.kthvalue(max(1, B // 16)).values)
                if score > best:
                    best, best_t = score, t_
            P["actor"]["ls_b"][o] = float(best_t - raw0[:, o].mean())
        b64 = (s64, a.double(), r.double(), s2.double(), d.double())
        bad = ~(clamp_margin(to64(P), b64, cc) > 1).all(1)
        if bool(bad.all()):
            continue
        good = torch.nonzero(~bad).reshape(-1)
        for n_, m in enumerate(torch.nonzero(bad).reshape(-1).tolist()):
            s[m] = s[good[n_ % len(good)]]
        raw = trunk(to64(P)["actor"], s.double())[1]
        eps[raw < EPS0_BELOW] = 0.0
        eps.mul_((Z_STEP_MAX / 3.0 / raw.clamp(CFG["ls_min"], CFG["ls_max"]).exp()).clamp(max=1.0).float())
        batch = (s, a, r, s2, d)
        establish_margins(P, batch, eps, chain, which="rest")
        P64, b64 = to64(P), tuple(x.double() for x in batch)
        R_ = rows(P64, b64, eps.double())
        raw = R_["raw"]
        if B >= 3 and not (bool((raw < CFG["ls_min"]).any()) and bool((raw > CFG["ls_max"]).any()) and bool(R_["inside"].bool().any())):
            continue
        if not margins_ok(P64, b64, eps.double(), chain, cc):
            continue
        return P, batch, eps, eps1, chain
    raise RuntimeError("no case with margins for %r" % ((obs_dim, hidden, hidden_v, B),))
