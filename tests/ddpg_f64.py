"""A float64 statement of one DDPG update (crowdnav.ddpg.Agent._update, ddpg.py:198-243 of the reference) for the tests of
cn_ddpg_update, built from the generic pieces of td3_f64 (forward passes, head derivatives, the propagated rounding bounds,
ReLU margins, the invertible Adam step).  What is DDPG's own: one critic and one target critic, y = r + (1 - d) gamma
Q_t(s2, pi_t(s2)) without target-policy noise, and the actor's gradient through the PRE-update critic -- so both gradients of
one update are functions of the same parameters and one kernel call yields them together.

The series (series_step; series(): the record adam_series.run walks): four updates with both optimisers' moments and step count
carried in float64 beside a learner -- the device handle, or EmulatedLearner's float32 formula on the CPU; SERIES_VARIANTS restate it
wrongly."""

import numpy as np
import torch

import adam_series as A
import td3_f64 as R

NETS = ("actor", "actor_t", "critic", "critic_t")
LOCAL = ("actor", "critic")


def new_params(obs_dim, hidden, gen, device="cpu"):
    """nn.Linear's default initialisation of the four networks, as float32 tensors."""
    P = R.new_params(obs_dim, hidden, gen, dtype=torch.float32, device=device)
    return dict(actor=P["actor"], actor_t=P["actor_t"], critic=P["q1"], critic_t=P["q1_t"])


def plant_dead_units(P, hidden):
    """td3_f64.plant_dead_units for the two local networks: unit 1 of layer 1 and unit hidden - 2 of layer 2 dead."""
    if hidden < 4:
        return {}
    dead = {}
    for n in LOCAL:
        u1, u2 = 1, hidden - 2
        P[n]["w1"][u1].zero_(); P[n]["b1"][u1] = 0
        P[n]["w2"][u2].zero_(); P[n]["b2"][u2] = 0
        dead[n] = (u1, u2)
    return dead


def _target_action(ft, nz, cfg, y_from):
    """pi_t(s2) and its magnitude; y_from="noise": the wrong variant with TD3's clipped target-policy noise added."""
    act, m_act = ft["act"], ft["m_act"]
    if y_from == "noise":
        noise = R.target_noise(nz, cfg)
        return act + noise, m_act + noise.abs()
    return act, m_act


def td_target(P, batch, cfg, y_from="single", nz=None):
    """y = r + (1 - d) gamma Q_t(s2, pi_t(s2)) and its magnitude.  Wrong variants for the discriminating checks: "twin" = TD3's
    min over two critics (the target critic and, as the second twin, the local critic on the same input), "noise" = TD3's
    target-policy noise nz (unit variance, scaled and clipped by cfg) added to the target action."""
    s, a, r, s2, d = batch
    ft = R.actor_fwd(P["actor_t"], s2, cfg)
    a2, m_a2 = _target_action(ft, nz, cfg, y_from)
    x2, xm2 = torch.cat([s2, a2], 1), torch.cat([s2.abs(), m_a2], 1)
    f = R._mlp(P["critic_t"], x2, xm2)
    qt = f["out"][:, 0]
    if y_from == "twin":
        qt = torch.minimum(qt, R._mlp(P["critic"], x2)["out"][:, 0])
    y = r + (1 - d) * cfg["gamma"] * qt
    return dict(y=y, m_y=r.abs() + (1 - d) * cfg["gamma"] * f["m_out"][:, 0], qt=qt, a2=a2)


def _critic_pass(ps, P, batch, cfg, y_from, nz):
    """The critic step's gradient (ddpg.py:219-230) as one td3_f64._Pass evaluation (exact or with perturbed roundings)."""
    s, a, r, s2, d = batch
    B = s.shape[0]
    ft = ps.mlp(P["actor_t"], s2, "actor_t")
    act, _ = ps.heads(ft["out"], cfg)
    if y_from == "noise":
        act = ps.ew(act + R.target_noise(nz, cfg))
    x2 = torch.cat([s2, act], 1)
    qt = ps.mlp(P["critic_t"], x2, "critic_t")["out"][:, 0]
    if y_from == "twin":
        qt = torch.minimum(qt, ps.mlp(P["critic"], x2, "critic_on_s2")["out"][:, 0])
    y = ps.ew(r + ps.ew((1 - d) * cfg["gamma"] * qt, 2.0))
    x = torch.cat([s, a], 1)
    f = ps.mlp(P["critic"], x, "critic")
    dq = ps.ew(2.0 * ps.ew(f["out"][:, 0] - y) / B, 2.0)
    g, _ = ps.backward(P["critic"], x, f, dq[:, None])
    return g


def critic_grads(P, batch, cfg, y_from="single", nz=None):
    """{g: autograd gradient of mean((Q(s, a) - y)^2) at P, bound: LAMBDA x propagated RMS, loss, t: the TD target's pieces}."""
    s, a, r, s2, d = batch
    with torch.no_grad():
        t = td_target(P, batch, cfg, y_from, nz)
    x = torch.cat([s, a], 1)
    _, bnd = R.propagated_bounds(lambda ps: _critic_pass(ps, P, batch, cfg, y_from, nz))
    g, loss = R._grad_of(lambda ps: ((R._mlp(ps, x)["out"][:, 0] - t["y"]) ** 2).mean(), P["critic"])
    return dict(g=g, bound=bnd, loss=loss, t=t)


def actor_grads(P, s, cfg, critic=None, N_mask=None):
    """d(-mean Q(s, pi(s)))/d actor (ddpg.py:216-217) through `critic` (default: P's, the pre-update one) -- td3_f64.actor_grads
    with the critic in Q1's place."""
    return R.actor_grads(P, s, cfg, q1=P["critic"] if critic is None else critic, N_mask=N_mask)


def establish_margins(P, batch, cfg, N, logit_scale=8.0, rescale=True):
    """td3_f64.establish_margins for DDPG's rows: the actor on s, actor_t on s2, the critic on (s, a) and (s, pi(s)), critic_t on
    (s2, pi_t(s2)).  Both policies' logits scaled to +-logit_scale first.  Modifies P's float32 tensors in place.
    rescale=False (re-establishing the margins between updates): only the hidden biases move."""
    s, a, r, s2, d = [x.double() for x in batch]
    rep = {}

    def net_margins(name, xs, xms):
        p = P[name]
        rep[name + ".1"] = R._layer_margins(p["w1"], p["b1"], xs, xms, N)
        p64 = {k: v.double() for k, v in p.items()}
        h = [R._mlp(p64, x, xm) for x, xm in zip(xs, xms)]
        rep[name + ".2"] = R._layer_margins(p["w2"], p["b2"], [f["h1"] for f in h], [f["m_h1"] for f in h], N)

    for name, x in (("actor", s), ("actor_t", s2)):
        net_margins(name, [x], [x.abs()])
        p64 = {k: v.double() for k, v in P[name].items()}
        lg = R._mlp(p64, x)["out"]
        if rescale:
            P[name]["w3"].mul_(logit_scale / max(float((lg - p64["b3"]).abs().max()), 1e-30))
    rows = _rows(P, (s, a, r, s2, d), cfg)
    net_margins("critic", *zip(*rows["critic"]))
    net_margins("critic_t", *zip(*rows["critic_t"]))
    return rep


def _rows(P, batch, cfg):
    s, a, r, s2, d = batch
    P64 = R.to64(P)
    fa = R.actor_fwd(P64["actor"], s, cfg)
    ft = R.actor_fwd(P64["actor_t"], s2, cfg)
    return dict(actor=[(s, s.abs())], actor_t=[(s2, s2.abs())],
                critic=[(torch.cat([s, a], 1), torch.cat([s, a], 1).abs()), (torch.cat([s, fa["act"]], 1), torch.cat([s.abs(), fa["m_act"]], 1))],
                critic_t=[(torch.cat([s2, ft["act"]], 1), torch.cat([s2.abs(), ft["m_act"]], 1))])


def margin_report(P, batch, cfg, N):
    """min over every non-dead unit and every row the kernel evaluates it on of |pre-activation| / bound (>= 1: no ambiguous mask)."""
    b = tuple(x.double() for x in batch)
    P64 = R.to64(P)
    worst = float("inf")
    for n, sets in _rows(P, b, cfg).items():
        p = P64[n]
        for x, xm in sets:
            f = R._mlp(p, x, xm)
            for z, m, w, bb in ((f["z1"], f["m_z1"], p["w1"], p["b1"]), (f["z2"], f["m_z2"], p["w2"], p["b2"])):
                live = ~R._is_dead(w, bb)
                r_ = (z.abs() / (N * R.U * m))[:, live]
                if r_.numel():
                    worst = min(worst, float(r_.min()))
    return worst


# ---- Adam across updates ------------------------------------------------------------------------------------------------------
SERIES_VARIANTS = ("frozen_bias_correction", "moments_not_carried", "betas_exchanged", "one_lr", "target_from_pre_step_weights")
# variant -> (the first update (from 0) at which it can differ, the networks it must be rejected on: some tensor of EACH)
SERIES_RULES = dict(frozen_bias_correction=(1, LOCAL), moments_not_carried=(1, LOCAL), betas_exchanged=(1, LOCAL), one_lr=(0, ("actor",)),
                    target_from_pre_step_weights=(0, ("actor_t", "critic_t")))
SERIES_SHAPES = ((45, 33, 40), (398, 256, 64))                   # (obs_dim, hidden, batch): test_gpu_ddpg's DISCRIMINATE
F32 = lambda x: float(np.float32(x))
SERIES_BETAS = ((0.5, 0.75), (F32(0.9), F32(0.999)))             # the product's as the config's float32 fields hold them
SERIES_CFG = dict(gamma=0.99, tau=2.0 ** -4, max_v=0.22, max_w=2.0, noise_std=0.25, noise_clip=0.5)
SERIES_LR = 2.0 ** -7
SERIES_UPDATES = 4
TARGET_OF = dict(actor="actor_t", critic="critic_t")
SERIES_CASES = ((SERIES_SHAPES[0], SERIES_BETAS[0]), (SERIES_SHAPES[0], SERIES_BETAS[1]), (SERIES_SHAPES[1], SERIES_BETAS[1]))     # the product shape once


def series_id(case):
    return "%s-b%g" % ("x".join(map(str, case[0])), round(case[1][0], 3))


def series_grads(P64, b64, cfg, N):
    """{critic, actor: dict(g, bound)} at P64: both gradients of one update, at the pre-update weights."""
    a = actor_grads(P64, b64[0], cfg, N_mask=N)
    assert a["flip_rows"] == 0
    return dict(critic=critic_grads(P64, b64, cfg), actor=a)


def series_hp(grads, betas, tau):
    """eps = a power of two >= twice the largest gradient element of the first update; lr = SERIES_LR x (the larger network's top
    |g|) / (its own), the actor's doubled if the two are equal."""
    top = {n: A.pow2_at_least(max(float(v.abs().max()) for v in grads[n]["g"].values())) for n in LOCAL}
    e_ = max(top.values())
    lr_c = SERIES_LR * e_ / top["critic"]
    lr_a = SERIES_LR * e_ / top["actor"]
    if lr_a == lr_c:
        lr_a *= 2.0
    return dict(lr_critic=lr_c, lr_actor=lr_a, beta1=betas[0], beta2=betas[1], eps=2.0 * e_, tau=tau)


def series_state(hp):
    return A.new_state(hp, ("critic", "actor"))


def series_step(state, P_pre, grads, hp, variant=None):
    """One update of the series: P_pre the pre-update weights in float64, grads = series_grads at them.  Both optimisers step on
    every update with one step count (adam_series.optimiser_turn / tensor_step); each target follows its stepped network.
    -> (predicted tensors, bounds) over the four networks, the targets at soft_bound + tau x the step bound."""
    tau = hp["tau"]
    state["t"] += 1
    pred, bound = {}, {}
    for net in LOCAL:
        o = state["opt"][net]
        t = A.optimiser_turn(o, state["t"], net, hp, ("critic", "actor"), variant)
        tg = TARGET_OF[net]
        pred[net], bound[net], pred[tg], bound[tg] = {}, {}, {}, {}
        for k in R.NAMES:
            w1, sb = A.tensor_step(o, state["gerr"], net, k, P_pre[net][k], grads[net]["g"][k], grads[net]["bound"][k], hp["eps"], t)
            pred[net][k], bound[net][k] = w1, sb
            src = P_pre[net][k] if variant == "target_from_pre_step_weights" else w1
            pred[tg][k], bound[tg][k] = R.soft_update(P_pre[tg][k], src, tau), R.soft_bound(P_pre[tg][k], src, tau) + tau * sb
    return pred, bound


class EmulatedLearner:
    """The stand-in for the device handle in the CPU checks: float64 gradients rounded to float32 into td3_f64.adam_f32_emulation
    with carried moments and one step count, the soft updates in float32."""

    def __init__(self, P, shape, hp, cfg=SERIES_CFG):
        self.P = {n: {k: v.detach().clone().float() for k, v in p.items()} for n, p in P.items()}
        self.hp, self.cfg, self.t, self.mom, self.N = hp, cfg, 0, {}, R.chain_length(*shape)

    def read(self):
        return {n: {k: v.clone() for k, v in p.items()} for n, p in self.P.items()}

    def write(self, P):
        self.P = {n: {k: v.clone() for k, v in p.items()} for n, p in P.items()}

    def update(self, batch):
        g = series_grads(R.to64(self.P), R.batch_double(batch), self.cfg, self.N)
        self.t += 1
        A.emulated_adam(self.P, self.mom, self.t, self.hp, [(n, R.NAMES) for n in LOCAL], lambda net, k: g[net]["g"][k])
        for net in LOCAL:
            for k in R.NAMES:
                self.P[TARGET_OF[net]][k] = A.soft_f32(self.P[TARGET_OF[net]][k], self.P[net][k], self.hp["tau"])

    def close(self):
        pass


def series_case(shape, device="cpu", cfg=SERIES_CFG):
    """test_gpu_ddpg.make_case's inputs (seed 5) with margins and planted dead units -> P, batch, N, dead, on `device`."""
    obs_dim, hidden, B = shape
    g = torch.Generator().manual_seed(5 + 1000 * hidden + B + 7)
    P = new_params(obs_dim, hidden, g, device=device)
    s = torch.randn((B, obs_dim), generator=g) * 0.5
    a = torch.stack([torch.rand(B, generator=g) * 0.22, torch.rand(B, generator=g) * 4 - 2], 1)
    r = 2 + 0.5 * torch.randn(B, generator=g)
    s2 = torch.randn((B, obs_dim), generator=g) * 0.5
    d = (torch.rand(B, generator=g) < 0.3).float()
    d[0], d[1] = 0, 1
    batch = tuple(x.float().to(device).contiguous() for x in (s, a, r, s2, d))
    dead = plant_dead_units(P, hidden)
    N = R.chain_length(*shape)
    establish_margins(P, batch, cfg, N)
    return P, batch, N, dead


def series(shape, betas, device="cpu", cfg=SERIES_CFG):
    """The record adam_series.run() walks for DDPG: series_case on `device` (a learner's read() / write() tensors live there
    too), both gradients at the pre-update weights, the margins re-established in place before every update after the first
    (only the hidden biases move), the planted dead units' weights bit for bit."""
    c = {}

    def case():
        P, c["batch"], c["N"], c["dead"] = series_case(shape, device, cfg)
        return P
    return A.series(
        tag="%s betas %.3g/%.4g" % ("x".join(map(str, shape)), betas[0], betas[1]), shape=shape, case=case,
        reference=lambda P: series_grads(R.to64(P), R.batch_double(c["batch"]), cfg, c["N"]),
        hp=lambda grads: series_hp(grads, betas, cfg["tau"]), lr_nets=("critic", "actor"), local=LOCAL, state=series_state,
        step=series_step,
        replant=lambda P: establish_margins(P, c["batch"], cfg, c["N"], rescale=False),
        margins_ok=lambda P: margin_report(P, c["batch"], cfg, c["N"]) >= 1.0,
        top=lambda grads: max(float(v.abs().max()) for n in LOCAL for v in grads[n]["g"].values()), inputs=lambda: (c["batch"],),
        frozen=lambda P: [x for n in LOCAL for x in A.dead_slices(P[n], c["dead"][n])], frozen_msg="a dead unit's weight moved",
        before=None, after=None, variants=SERIES_VARIANTS, rules=SERIES_RULES, report=NETS, alias=None)
