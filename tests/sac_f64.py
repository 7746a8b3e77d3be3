"""TEST INFRASTRUCTURE.  A float64 restatement of what cn_sac_update computes per row (sac.py:253-272 of the reference): the
heads, the sample, the double squash, log_prob, the four network outputs, the three losses and the per-row loss gradients, with
the gradients BY FORMULA (rows()), and the whole update -- those and every weight gradient of Q, V and the actor -- as a
td3_f64._Pass evaluation (run()) whose perturbed runs give the error bounds (reference()).  tests/test_sac_f64_helpers.py holds
both to torch.autograd on the reference's loss expressions.

cn_sac_act's statement (act_pass / act_reference) shares run()'s head, clamp, sample and squash statements (_heads, _squash);
act_case builds its inputs with margins on every row from make_case's own pieces; box_muller_draw states the on-device draw.

Parameters are dicts {net: {name: tensor}} like tests/td3_f64.py's: actor = w1, b1, w2, b2, mean_w, mean_b, ls_w, ls_b;
q, v, v_t = td3_f64.NAMES.  `variant` restates the update WRONGLY in one named way (the discrimination tests).

The series (series_step; series(): the record adam_series.run walks): four updates with Adam's moments, the shared step count and
V's soft update carried in float64 beside a learner -- the device handle, or EmulatedLearner's float32 formula on the CPU -- whose
weights are read back before and after every update; SERIES_VARIANTS restate the series wrongly, one way at a time."""
import functools
import math

import numpy as np
import torch

import adam_series as A
import td3_f64 as R
from actor_f64 import uniforms
from sampling_f64 import angle_f32, noise_hash
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


def _heads(ps, pa, h2, eps, cfg=CFG, deterministic=False, variant=None):
    """Both heads, the clamp, std and the sample from the trunk's output h2, statement by statement as sac_squash computes them
    (cn_sac_update's head kernel and cn_sac_act share it) -> mean, raw, ls, sd, inside, z, t.  The clamp classes are those of the
    exact run.  deterministic: z = mean, no rounding.  variant: one of ACT_VARIANTS' wrong heads (the squash's are _squash's)."""
    c = cfg
    mw, lw, mb, lb = pa["mean_w"], pa["ls_w"], pa["mean_b"], pa["ls_b"]
    if variant == "heads_swapped":
        mw, lw = lw, mw
    if variant == "no_head_bias":
        mb, lb = torch.zeros_like(mb), torch.zeros_like(lb)
    if variant == "second_row_of_head_is_first":
        mw, lw = mw[[0, 0]], lw[[0, 0]]
    mean, raw = _lin(ps, h2, mw, mb), _lin(ps, h2, lw, lb)
    if ps.gen is None:
        ps.masks["lo"], ps.masks["hi"] = (raw < c["ls_min"]).to(raw.dtype), (raw > c["ls_max"]).to(raw.dtype)
        if variant == "unclamped_log_std":
            ps.masks["lo"], ps.masks["hi"] = torch.zeros_like(raw), torch.zeros_like(raw)
    lo, hi = ps.masks["lo"], ps.masks["hi"]
    inside = 1 - lo - hi
    ls = raw * inside + lo * c["ls_min"] + hi * c["ls_max"]
    sd = ls if variant == "std_is_log_std" else ps.ew(ls.exp(), 4.0)
    if deterministic:
        z = mean
    else:
        e = eps.flip(1) if variant == "eps_swapped" else eps
        step = ps.ew(e * sd)
        z = ps._noise(step + mean, R.U * (step + mean).abs() * (step != 0))          # eps = 0: z = mean exactly
    t = ps.ew(torch.tanh(z), 4.0).clamp(-1.0, 1.0)                            # tanhf never leaves [-1, 1]
    return mean, raw, ls, sd, inside, z, t


def _squash(ps, t, cfg=CFG, variant=None):
    """The second squash (SAC:90-91) of t = tanh z."""
    c = cfg
    if variant == "single_squash":
        return ps.ew(torch.stack([t[:, 0] * c["max_v"], t[:, 1] * c["max_w"]], 1))
    if variant == "squashes_swapped":
        return ps.ew(torch.stack([torch.tanh(t[:, 0]) * c["max_v"], torch.sigmoid(t[:, 1]) * c["max_w"]], 1), 4.0)
    return ps.ew(torch.stack([torch.sigmoid(t[:, 0]) * c["max_v"], torch.tanh(t[:, 1]) * c["max_w"]], 1), 4.0)


def run(ps, P, batch, eps, cfg=CFG, variant=None, eps_first=None):
    """One update as a td3_f64._Pass evaluation, operation by operation as sac_head_kernel / sac_loss_kernel and the GEMM jobs
    compute it (exact with _Pass(), or with every rounding perturbed: td3_f64.propagated_bounds).  -> the per-row quantities
    of KEYS and the weight gradients of Q, V and the actor as (net, name).  The ReLU masks and the clamp classes are those of
    the exact run (the margins guarantee that float32 decides them alike)."""
    s, a, r, s2, d = batch
    B, c, pa = s.shape[0], cfg, P["actor"]
    z1 = _lin(ps, s, pa["w1"], pa["b1"]); m1 = ps.mask("actor.1", z1); h1 = z1 * m1
    z2 = _lin(ps, h1, pa["w2"], pa["b2"]); m2 = ps.mask("actor.2", z2); h2 = z2 * m2
    e = eps_first if variant == "first_sample" else eps
    mean, raw, ls, sd, inside, z, t = _heads(ps, pa, h2, e, c)
    dz, var = ps.ew(z - mean), ps.ew(sd * sd)
    om = ps.ew(ps.ew(1 - ps.ew(t * t)) + c["logp_eps"])                       # 1 - t^2 cancels: t^2's rounding lands on it absolutely
    terms = torch.stack([-ps.ew(ps.ew(dz * dz) / (2 * var), 2.0), -ps.ew(sd.log(), 4.0), torch.full_like(z, -0.5 * math.log(2 * math.pi)),
                         -ps.ew(om.log(), 4.0)], 2)
    logp = ps._noise(terms.sum((1, 2)), 8 * R.U * terms.abs().sum((1, 2)))
    a_new = _squash(ps, t, c, "single_squash" if variant == "single_squash" else None)
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


def reference(P, batch, eps, cfg=CFG, variant=None, eps_first=None, device=None):
    """(float64 values, bounds) of everything run() returns: the bounds are td3_f64.propagated_bounds' LAMBDA x the RMS change over
    perturbed runs -- they follow the float32 error of each element (an exact zero has bound zero), not its worst case.
    device: the inputs, of any float type, are taken to float64 on it first (the GPU tests' "cuda"); the results are on the CPU."""
    if device is not None:
        d = lambda x: None if x is None else x.double().to(device)
        P, batch, eps, eps_first = {n: {k: d(v) for k, v in p.items()} for n, p in P.items()}, tuple(d(x) for x in batch), d(eps), d(eps_first)
    want, bound = R.propagated_bounds(lambda ps: run(ps, P, batch, eps, cfg, variant, eps_first))
    return {k: v.cpu() for k, v in want.items()}, {k: v.cpu() for k, v in bound.items()}


def cuda(batch):
    return tuple(x.float().cuda().contiguous() for x in batch)


SCALE_ERR = 1e-3                               # the uniform gradient scale error the discrimination tests must reject


def handle_config(P, shape, lr=3e-4, replay=None, soft_update=0, tau=5e-3, seed=7, **over):
    """The cn_sac_config of a raw handle (learner_handle.LearnerHandle("sac", ..)) on the float32 device tensors P."""
    from learner_handle import lib, mlp_struct, ring_fields
    c = CFG
    kw = dict(obs_dim=shape[0], hidden=shape[1], hidden_v=shape[2], batch=shape[3], gamma=c["gamma"], tau=tau, lr_actor=lr, lr_v=lr,
              lr_q=lr, beta1=0.9, beta2=0.999, eps=1e-8, max_v=c["max_v"], max_w=c["max_w"], log_std_min=c["ls_min"],
              log_std_max=c["ls_max"], mean_lambda=c["mean_lambda"], std_lambda=c["std_lambda"], z_lambda=c["z_lambda"],
              logp_eps=c["logp_eps"], soft_update=soft_update, reserved=0, actor=mlp_struct(P["actor"], ACTOR_NAMES, "CnSacActor"),
              seed=seed, **{n: mlp_struct(P[n], NAMES) for n in ("q", "v", "v_t")})
    kw.update(ring_fields(replay)); kw.update(over)
    return lib()[0].CnSacConfig(**kw)


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


def relu_margins_ok(p, x, chain):
    """Both hidden layers of p on the rows x: every pre-activation farther from zero than chain EPS32 x its magnitude -- but for a
    planted dead unit (zero weight row, zero bias: td3_f64.plant_dead_units), whose pre-activation is exactly 0 in any order."""
    u = chain * EPS32
    z1 = x @ p["w1"].T + p["b1"]; a1 = x.abs() @ p["w1"].abs().T + p["b1"].abs()
    h1 = torch.relu(z1)
    z2 = h1 @ p["w2"].T + p["b2"]; a2 = a1 @ p["w2"].abs().T + p["b2"].abs()
    d1, d2 = R._is_dead(p["w1"], p["b1"]), R._is_dead(p["w2"], p["b2"])
    return bool(((z1.abs() > u * a1) | d1).all()) and bool(((z2.abs() > u * a2) | d2).all())


def actor_margins_ok(pa, s, chain, clamp_chain):
    """margins_ok's actor part: the trunk's ReLU masks and every clamp decision of every row of s."""
    return relu_margins_ok(pa, s, chain) and bool((clamp_margin({"actor": pa}, (s,), clamp_chain) > 1).all())


def margins_ok(P, batch, eps, chain, clamp_chain=None):
    """No ReLU mask and no clamp decision may differ between float32 and float64: every pre-activation and every raw log_std keeps
    a distance from its threshold above the forward-error bound of its own dot product."""
    s, a, r, s2, d = batch
    R_ = rows(P, batch, eps)
    return actor_margins_ok(P["actor"], s, chain, clamp_chain or chain) and all(relu_margins_ok(p, x, chain) for p, x in (
        (P["q"], torch.cat([s, a], 1)), (P["q"], torch.cat([s, R_["a_new"]], 1)), (P["v"], s), (P["v_t"], s2)))


def establish_margins(P, batch, eps, N, which="all"):
    """Shift every hidden unit's bias (td3_f64._layer_margins), network by network in the order the rows depend on each other:
    the actor on s, Q on (s, a) and (s, a_new), V on s, V_t on s2.  Modifies P's float32 tensors in place."""
    s = batch[0].double()

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
    s, a, r, s2, d = [x.double() for x in batch]
    R_ = rows(to64(P), (s, a, r, s2, d), eps.double())
    m_act = torch.full_like(R_["a_new"], 4.0)                  # |a_new| <= 2 and its error's magnitude, generously
    net("q", [torch.cat([s, a], 1), torch.cat([s, R_["a_new"]], 1)], [torch.cat([s, a], 1).abs(), torch.cat([s.abs(), m_act], 1)])
    net("v", [s], [s.abs()])
    net("v_t", [s2], [s2.abs()])


def plant_clamp_head(pa, s, cc):
    """make_case's log_std head, in place on the float32 actor pa and the rows s: per output one large weight on the second-layer
    unit with the largest spread over the rows, the bias where the two clamp edges are clearest, rows still within the bound of
    an edge replaced by copies of rows that are not.  False (pa's head may have changed) where it cannot be built: fewer than two
    rows, no unit with spread, or every row near an edge."""
    B = s.shape[0]
    p64 = {k_: v.double() for k_, v in pa.items()}
    s64 = s.double()
    h2 = trunk(p64, s64)[3]
    a2 = (s64.abs() @ p64["w1"].abs().T + p64["b1"].abs()) @ p64["w2"].abs().T + p64["b2"].abs()
    spread = h2.max(0).values - h2.min(0).values
    units = torch.argsort(spread / a2.max(0).values, descending=True)[:2].tolist()
    if B < 2 or float(spread[units[0]]) <= 0:
        return False
    for o in range(2):
        j = units[o % len(units)]
        if float(spread[j]) > 0:
            pa["ls_w"][o, j] = (44.0 if o == 0 else -44.0) / float(spread[j])
    p64 = {k_: v.double() for k_, v in pa.items()}
    raw0 = h2 @ p64["ls_w"].T
    ra = a2 @ p64["ls_w"].abs().T + 22.0
    ts = torch.linspace(-12.0, -6.0, 241).double()
    for o in range(2):           # the first of the 241 centres at which the (B // 16)-th smallest clearance is largest
        x = (raw0[:, o] - raw0[:, o].mean())[:, None] + ts[None, :]
        clear = torch.minimum((x - CFG["ls_min"]).abs(), (x - CFG["ls_max"]).abs()) / ra[:, o, None]
        best_t = float(ts[clear.kthvalue(max(1, B // 16), 0).values.argmax()])
        pa["ls_b"][o] = float(best_t - raw0[:, o].mean())
    return replace_rows_near_an_edge(pa, s, cc)


def replace_rows_near_an_edge(pa, s, cc):
    """Rows of s (in place) with a raw log_std within its bound of a clamp edge become copies of rows without; False if all are."""
    bad = ~(clamp_margin({"actor": {k_: v.double() for k_, v in pa.items()}}, (s.double(),), cc) > 1).all(1)
    if bool(bad.all()):
        return False
    good = torch.nonzero(~bad).reshape(-1)
    for n_, m in enumerate(torch.nonzero(bad).reshape(-1).tolist()):
        s[m] = s[good[n_ % len(good)]]
    return True


def tame_eps(pa, s, eps):
    """make_case's eps treatment, in place: zero where the raw log_std is below EPS0_BELOW, scaled so that |eps| std <= Z_STEP_MAX."""
    raw = trunk({k_: v.double() for k_, v in pa.items()}, s.double())[1]
    eps[raw < EPS0_BELOW] = 0.0
    eps.mul_((Z_STEP_MAX / 3.0 / raw.clamp(CFG["ls_min"], CFG["ls_max"]).exp()).clamp(max=1.0).float())


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
        if not plant_clamp_head(P["actor"], s, cc):
            continue
        tame_eps(P["actor"], s, eps)
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


# ---- cn_sac_act ---------------------------------------------------------------------------------------------------------------
ACT_KEYS = ("mean", "log_std", "z", "twist")
ACT_VARIANTS = ("single_squash", "squashes_swapped", "unclamped_log_std", "std_is_log_std", "eps_swapped", "heads_swapped", "no_head_bias",
                "second_row_of_head_is_first")
# the 16-unit tile, the 32-unit padding of hidden, the head's four lanes (units part mod 4), the LDS limit
ACT_HIDDEN = (1, 15, 16, 17, 31, 32, 33, 300, 479, 480)
ACT_D = (1, 3, 15, 16, 17, 127, 128, 129, 363)        # the ragged block of 16 inputs, eight blocks in flight
ACT_N = (1, 15, 16, 17, 33)                           # rows against the 16-row workgroup
ACT_LARGE = (32, 17, 65541)                           # (hidden, D, n): more than 4096 workgroups, a ragged last one
ACT_DISCRIMINATE = ((32, 46, 16), (33, 45, 40), (256, 363, 64))       # (hidden, D, n)


def act_pass(ps, actor, obs, eps, deterministic, cfg=CFG, variant=None):
    """What sac_act_kernel computes per row (Agent.act, SAC:206-229) as a td3_f64._Pass evaluation: the trunk, _heads (both heads,
    the clamp, exp, z = eps std + mean or z = mean, tanh), _squash, the clip to [0, max_v] x [-max_w, max_w] -- run()'s own
    statements and roundings.  actor, obs [n, obs_dim], eps [n, 2]: float64.  -> mean, log_std (clamped), z, twist."""
    c = cfg
    z1 = _lin(ps, obs, actor["w1"], actor["b1"]); h1 = z1 * ps.mask("actor.1", z1)
    z2 = _lin(ps, h1, actor["w2"], actor["b2"]); h2 = z2 * ps.mask("actor.2", z2)
    mean, raw, ls, sd, inside, z, t = _heads(ps, actor, h2, eps, c, deterministic, variant)
    a = _squash(ps, t, c, variant)
    lo = torch.tensor([0.0, -c["max_w"]], dtype=a.dtype, device=a.device)
    hi = torch.tensor([c["max_v"], c["max_w"]], dtype=a.dtype, device=a.device)
    return dict(mean=mean, log_std=ls, z=z, twist=torch.maximum(torch.minimum(a, hi), lo))


def act_reference(actor, obs, eps, deterministic, cfg=CFG, variant=None):
    """(float64 values, bounds) of act_pass: td3_f64.propagated_bounds.  A clamped log_std has bound zero."""
    return R.propagated_bounds(lambda ps: act_pass(ps, actor, obs, eps, deterministic, cfg, variant))


def act_classes(actor, obs):
    """(below, inside, above): which raw log_std elements the float64 actor clamps at log_std_min, leaves, clamps at log_std_max."""
    raw = trunk({k: v.double() for k, v in actor.items()}, obs.double())[1]
    return raw < CFG["ls_min"], (raw >= CFG["ls_min"]) & (raw <= CFG["ls_max"]), raw > CFG["ls_max"]


def act_promises_classes(hidden, n):
    return hidden >= 15 and n >= 15


@functools.lru_cache(maxsize=None)
def _act_case(hidden, obs_dim, n, seed):
    cc = clamp_chain(obs_dim, hidden)          # >= the roundings on the way to any pre-activation of the trunk as well
    need = act_promises_classes(hidden, n)
    for k in range(60):
        g = torch.Generator().manual_seed(1000 * seed + k + 31 * hidden + 977 * obs_dim + 7919 * n)
        pa = new_params(obs_dim, hidden, 1, g)["actor"]
        s = torch.randn((n, obs_dim), generator=g) * 0.5
        eps = torch.randn((n, 2), generator=g).clamp(-3, 3)
        establish_margins({"actor": pa}, (s,), None, cc, which="actor")
        plain = {k_: pa[k_].clone() for k_ in ("ls_w", "ls_b")}
        if not plant_clamp_head(pa, s, cc):
            # one row, or a trunk whose output is the same on every row: the nn.Linear-like head as drawn, far inside the clamp
            pa.update(plain)
            if need or not replace_rows_near_an_edge(pa, s, cc):
                continue
        if (hidden + obs_dim + n) % 2:       # plant_clamp_head's output 0 reaches the upper edge alone, output 1 the lower: every
            pa["ls_w"], pa["ls_b"] = pa["ls_w"][[1, 0]].contiguous(), pa["ls_b"][[1, 0]].contiguous()      # other case the other way
        tame_eps(pa, s, eps)
        below, inside, above = act_classes(pa, s)
        if need and not (bool(below.any()) and bool(inside.any()) and bool(above.any())):
            continue
        if not actor_margins_ok({k_: v.double() for k_, v in pa.items()}, s.double(), cc, cc):
            continue
        return pa, s, eps
    raise RuntimeError("no act case with margins for %r" % ((hidden, obs_dim, n),))


def act_case(hidden, obs_dim, ld, n, seed=0):
    """cn_sac_act's inputs: actor parameters (float32 values), obs [n, ld] with NaN in columns obs_dim .. ld - 1 (the same values
    whatever ld) and eps [n, 2], such that actor_margins_ok holds at clamp_chain(obs_dim, hidden) for EVERY row: no ReLU mask
    and no clamp decision differs between float32 and float64.  Built as make_case builds its actor: establish_margins on the
    trunk, plant_clamp_head, tame_eps.  hidden >= 15 and n >= 15: elements clamped at -20, clamped at 2 and inside all occur.
    Smaller: the same head where it can be built, else (one row, or no second-layer unit that differs between the rows) the
    nn.Linear-like head as drawn, which stays inside the clamp; margins in either case."""
    pa, s, eps = _act_case(hidden, obs_dim, n, seed)
    obs = torch.full((n, ld), float("nan"))
    obs[:, :obs_dim] = s
    return {k: v.clone() for k, v in pa.items()}, obs, eps.clone()


# ---- the draw -----------------------------------------------------------------------------------------------------------------
def box_muller_draw(seed, counter, rows):
    """The documented draw of row `rows` of call `counter`, under td3_prep_kernel's and sac_act_kernel's key
    sampling_f64.noise_hash: eps = (r cos a, r sin a), r = sqrt(-2 ln u1), a = fl32(6.28318530718f u2) -- the angle as the kernel
    rounds it (sampling_f64.angle_f32), everything else in float64 on actor_f64.uniforms' exact u1 in (0, 1] (1 at k = 2^24 - 1
    alone, where eps = 0) and u2 in [0, 1).  -> float64 [len(rows), 2]."""
    u1, u2 = uniforms(noise_hash(seed, counter, None, rows))
    r, a = np.sqrt(-2.0 * np.log(u1)), angle_f32(u2)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


# ---- Adam across updates ------------------------------------------------------------------------------------------------------
SERIES_VARIANTS = ("frozen_bias_correction", "moments_not_carried", "betas_exchanged", "head_moments_exchanged", "one_lr",
                   "target_from_pre_step_v", "pull_before_adam", "pull_not_seen_by_moments")
# variant -> (the soft_update modes it exists in, the first update (from 0) at which it can differ, the networks it concerns: it
# must be rejected on at least one tensor of EACH)
SERIES_RULES = dict(frozen_bias_correction=((0, 1), 1, ("q", "v", "actor")), moments_not_carried=((0, 1), 1, ("q", "v", "actor")),
                    betas_exchanged=((0, 1), 1, ("q", "v", "actor")), head_moments_exchanged=((0, 1), 1, ("heads",)),
                    one_lr=((0, 1), 0, ("v", "actor")), target_from_pre_step_v=((1,), 0, ("v_t",)), pull_before_adam=((0,), 0, ("v",)),
                    pull_not_seen_by_moments=((0,), 1, ("v",)))
HEADS = ("mean_w", "mean_b", "ls_w", "ls_b")
SERIES_SHAPES = ((46, 32, 2, 16), (45, 33, 3, 40), (45, 24, 17, 40))       # (obs_dim, hidden, hidden_v, batch); both soft_update modes
SERIES_PRODUCT = (363, 256, 2, 64)                                         # once
F32 = lambda x: float(np.float32(x))
# carried moments weigh most at 0.5 / 0.75; the product's 0.9 / 0.999 AS THE CONFIG'S FLOAT32 FIELDS HOLD THEM (the kernel's
# 1 - beta and its tick's beta^t both start from that float32 value): the bias corrections are x10 and x1000 at t = 1
SERIES_BETAS = ((0.5, 0.75), (F32(0.9), F32(0.999)))
SERIES_TAU = 2.0 ** -4
SERIES_LR = 2.0 ** -7            # the largest step of an element of any network, about: each lr is this x eps / (2 top |g| of its net)
SERIES_UPDATES = 4
NET_NAMES = (("q", NAMES), ("v", NAMES), ("actor", ACTOR_NAMES))
# (shape, betas, soft_update, clamp_all): what the GPU series tests run and the CPU power test runs first.  The product shape once,
# as the product is configured (soft_update 0); one case with log_std output 1 clamped on every row (its head rows' exact zeros)
SERIES_CASES = tuple((s_, b_, m_, False) for s_ in SERIES_SHAPES for b_ in SERIES_BETAS for m_ in (0, 1)) + (
    (SERIES_PRODUCT, SERIES_BETAS[1], 0, False), (SERIES_SHAPES[1], SERIES_BETAS[1], 1, True))


def series_id(case):
    shape, betas, mode, clamp_all = case
    return "%s-b%g-soft%d%s" % ("x".join(map(str, shape)), round(betas[0], 3), mode, "-clamped" if clamp_all else "")


def series_hp(want, betas, soft_update, tau=SERIES_TAU):
    """The hyper-parameters of a series from the first update's float64 gradients `want`: eps = a power of two >= twice the
    largest gradient element; each optimiser's lr = SERIES_LR x (the largest network's top |g|) / (its own), powers of two,
    a later one doubled until the three differ (one_lr must show on V and on the actor)."""
    top = {n: A.pow2_at_least(max(float(want[k].abs().max()) for k in GRADS if k[0] == n)) for n in ("q", "v", "actor")}
    e_ = max(top.values())
    lr, seen = {}, set()
    for n in ("q", "v", "actor"):
        x = SERIES_LR * e_ / top[n]
        while x in seen:
            x *= 2.0
        seen.add(x)
        lr[n] = x
    return dict(lr_q=lr["q"], lr_v=lr["v"], lr_actor=lr["actor"], beta1=betas[0], beta2=betas[1], eps=2.0 * e_, tau=tau, soft_update=soft_update)


def series_state(hp):
    """adam_series.new_state for Q, V and the actor, and (pull_not_seen_by_moments) V's last un-pulled step."""
    return dict(A.new_state(hp, ("q", "v", "actor")), unpulled=None)


def series_step(state, P_pre, batch, eps, cfg, hp, variant=None, ref=None):
    """One update of the series.  P_pre: the pre-update weights in float64 (as read back from the learner); ref: reference()'s
    (gradients, bounds) at P_pre (computed here if None).  Advances `state` and returns (predicted post-update tensors, bounds),
    both {net: {name: tensor}} over q, v, v_t and actor.

    Q and the actor: Adam64's step at td3_f64.adam_step_bound, gerr the running maximum of the gradient bounds so far.
    soft_update 1: V the same, V_t = soft_update(V_t, V', tau) at soft_bound + tau x V's step bound.
    soft_update 0: V = soft_update(V', V_t, tau) at (1 - tau) x V's step bound + soft_bound; V_t keeps every bit (bound 0).
    variant: one of SERIES_VARIANTS."""
    if ref is None:
        ref = reference(P_pre, batch, eps, cfg)
    want, Bd = ref
    tau, mode = hp["tau"], hp["soft_update"]
    if variant == "pull_not_seen_by_moments" and state["unpulled"] is not None:       # the gradients at V as it was before the last pull
        alt = dict(P_pre, v={k: P_pre["v"][k] + state["unpulled"][k] for k in NAMES})
        want = run(R._Pass(), alt, batch, eps, cfg)
    state["t"] += 1
    pred, bound = {}, {}
    for net, names in NET_NAMES:
        o = state["opt"][net]
        t = A.optimiser_turn(o, state["t"], net, hp, ("q", "v", "actor"), variant)
        if variant == "head_moments_exchanged" and net == "actor":
            for a_, b_ in (("mean_w", "ls_w"), ("mean_b", "ls_b")):
                for mom in (o.m, o.v):
                    if a_ in mom:
                        mom[a_], mom[b_] = mom[b_], mom[a_]
        pred[net], bound[net] = {}, {}
        for k in names:
            w0 = P_pre[net][k]
            if net == "v" and variant == "pull_before_adam":
                w0 = R.soft_update(w0, P_pre["v_t"][k], tau)
            pred[net][k], bound[net][k] = A.tensor_step(o, state["gerr"], net, k, w0, want[(net, k)], Bd[(net, k)], hp["eps"], t)
    pred["v_t"], bound["v_t"] = {}, {}
    unpulled = {}
    for k in NAMES:
        v1, sb, t0 = pred["v"][k], bound["v"][k], P_pre["v_t"][k]
        if mode == 1:
            src = P_pre["v"][k] if variant == "target_from_pre_step_v" else v1
            pred["v_t"][k], bound["v_t"][k] = R.soft_update(t0, src, tau), R.soft_bound(t0, src, tau) + tau * sb
        else:
            pred["v_t"][k], bound["v_t"][k] = t0, torch.zeros_like(t0)
            if variant != "pull_before_adam":
                pred["v"][k], bound["v"][k] = R.soft_update(v1, t0, tau), (1 - tau) * sb + R.soft_bound(v1, t0, tau)
            unpulled[k] = v1 - pred["v"][k]
    state["unpulled"] = unpulled if mode == 0 else None
    return pred, bound


class EmulatedLearner:
    """The stand-in for the device handle in the CPU checks: float64 gradients rounded to float32 into td3_f64.adam_f32_emulation
    (the kernel's formula in float32) with carried moments and one step count, V's soft update in float32."""

    def __init__(self, P, shape, hp):
        self.P = {n: {k: v.detach().clone().float() for k, v in p.items()} for n, p in P.items()}
        self.hp, self.t, self.mom = hp, 0, {}

    def read(self):
        return {n: {k: v.clone() for k, v in p.items()} for n, p in self.P.items()}

    def write(self, P):
        for n in P:
            for k in P[n]:
                self.P[n][k].copy_(P[n][k])

    def update(self, batch, eps):
        g = run(R._Pass(), to64(self.P), tuple(x.double() for x in batch), eps.double())
        self.t += 1
        A.emulated_adam(self.P, self.mom, self.t, self.hp, NET_NAMES, lambda net, k: g[(net, k)])
        moved, toward = ("v_t", "v") if self.hp["soft_update"] == 1 else ("v", "v_t")
        for k in NAMES:
            self.P[moved][k] = A.soft_f32(self.P[moved][k], self.P[toward][k], self.hp["tau"])

    def close(self):
        pass


def series_case(shape, clamp_all=False):
    """make_case plus a planted dead unit in each hidden layer of Q (td3_f64.plant_dead_units) and, with clamp_all, log_std output 1
    pushed 60 below on every row: clamped at log_std_min everywhere.  -> P, batch (a list: its s is edited in place between
    updates), eps, chain, clamp chain, the dead units."""
    P, batch, eps, _, chain = make_case(*shape)
    cc = clamp_chain(shape[0], shape[1])
    dead = R.plant_dead_units(P, shape[1], nets=("q",))
    if clamp_all:
        P["actor"]["ls_b"][1] -= 60.0
        assert replace_rows_near_an_edge(P["actor"], batch[0], cc)
        tame_eps(P["actor"], batch[0], eps)
    establish_margins(P, batch, eps, chain, which="rest")
    return P, list(batch), eps, chain, cc, dead


def _replant(P, batch, eps, chain, cc):
    """Before every update after the first, on the weights as they now stand (float32, in place): the actor's ReLU margins, rows
    near a clamp edge replaced, eps tamed, then the margins of Q, V and V_t on the rows that follow from those."""
    establish_margins(P, batch, eps, chain, which="actor")
    assert replace_rows_near_an_edge(P["actor"], batch[0], cc), "every row near a clamp edge"
    tame_eps(P["actor"], batch[0], eps)
    establish_margins(P, batch, eps, chain, which="rest")


def series(shape, betas, soft_update, clamp_all=False, device="cpu"):
    """The record adam_series.run() walks for SAC: series_case, reference() on `device`, a fresh tamed eps per update (seeded by
    the shape), the margins re-planted before every update after the first; Q's planted dead units and, with clamp_all, the
    log_std head's row 1 bit for bit; V_t bit for bit under soft_update 0."""
    tag = "%s betas %.3g/%.4g soft_update %d%s" % ("x".join(map(str, shape)), betas[0], betas[1], soft_update, " clamp_all" if clamp_all else "")
    variants = [v for v in SERIES_VARIANTS if soft_update in SERIES_RULES[v][0]]
    gen = torch.Generator().manual_seed(4242 + shape[1] + shape[3])
    c = {}

    def case():
        P, c["batch"], c["eps"], c["chain"], c["cc"], c["dead"] = series_case(shape, clamp_all)
        c["vt0"] = {k: v.clone() for k, v in P["v_t"].items()}
        return P

    def replant(P):
        c["eps"] = torch.randn(c["eps"].shape, generator=gen).clamp(-3, 3)
        _replant(P, c["batch"], c["eps"], c["chain"], c["cc"])

    def b64():
        return tuple(x.double() for x in c["batch"])

    def before(u, ref):
        if clamp_all:
            assert bool((ref[0]["raw"][:, 1] < CFG["ls_min"]).all()) and bool((ref[0]["dl"][:, 3] == 0).all())

    def after(u, post):
        if soft_update == 0:
            assert all(torch.equal(post["v_t"][k], c["vt0"][k]) for k in NAMES), (tag, u, "V_t moved")
    return A.series(
        tag=tag, shape=shape, case=case, reference=lambda P: reference(P, c["batch"], c["eps"], device=device),
        hp=lambda ref: series_hp(ref[0], betas, soft_update), lr_nets=("q", "v", "actor"), local=("q", "v", "actor"), state=series_state,
        step=lambda state, P64, ref, hp, var: series_step(state, P64, b64(), c["eps"].double(), CFG, hp, variant=var, ref=ref),
        replant=replant, margins_ok=lambda P: margins_ok(to64(P), b64(), c["eps"].double(), c["chain"], c["cc"]),
        top=lambda ref: max(float(ref[0][k].abs().max()) for k in GRADS), inputs=lambda: (tuple(c["batch"]), c["eps"]),
        frozen=lambda P: A.dead_slices(P["q"], c["dead"]["q"]) + ([P["actor"]["ls_w"][1], P["actor"]["ls_b"][1]] if clamp_all else []),
        frozen_msg="a weight with zero gradient and zero moments moved", before=before, after=after, variants=variants,
        rules={v: SERIES_RULES[v][1:] for v in variants}, report=("q", "v", "v_t", "actor"), alias={"heads": ("actor", HEADS)})
