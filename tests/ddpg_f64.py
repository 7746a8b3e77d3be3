"""A float64 statement of one DDPG update (crowdnav.ddpg.Agent._update, ddpg.py:198-243 of the reference) for the tests of
cn_ddpg_update, built from the generic pieces of td3_f64 (forward passes, head derivatives, the propagated rounding bounds,
ReLU margins, the invertible Adam step).  What is DDPG's own: one critic and one target critic, y = r + (1 - d) gamma
Q_t(s2, pi_t(s2)) without target-policy noise, and the actor's gradient through the PRE-update critic -- so both gradients of
one update are functions of the same parameters and one kernel call yields them together.

The series (series_step, series_run): four updates with both optimisers' moments and step count carried in float64 beside a
learner -- the device handle, or EmulatedLearner's float32 formula on the CPU; SERIES_VARIANTS restate it wrongly."""
import math

import numpy as np
import torch

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


def _pow2_at_least(x):
    return 2.0 ** math.ceil(math.log2(max(x, 2.0 ** -60)))


def series_grads(P64, b64, cfg, N):
    """{critic, actor: dict(g, bound)} at P64: both gradients of one update, at the pre-update weights."""
    a = actor_grads(P64, b64[0], cfg, N_mask=N)
    assert a["flip_rows"] == 0
    return dict(critic=critic_grads(P64, b64, cfg), actor=a)


def series_hp(grads, betas, tau):
    """eps = a power of two >= twice the largest gradient element of the first update; lr = SERIES_LR x (the larger network's top
    |g|) / (its own), the actor's doubled if the two are equal."""
    top = {n: _pow2_at_least(max(float(v.abs().max()) for v in grads[n]["g"].values())) for n in LOCAL}
    e_ = max(top.values())
    lr_c = SERIES_LR * e_ / top["critic"]
    lr_a = SERIES_LR * e_ / top["actor"]
    if lr_a == lr_c:
        lr_a *= 2.0
    return dict(lr_critic=lr_c, lr_actor=lr_a, beta1=betas[0], beta2=betas[1], eps=2.0 * e_, tau=tau)


def series_state(hp):
    mk = lambda lr: R.Adam64(lr, hp["beta1"], hp["beta2"], hp["eps"])
    return dict(t=0, opt=dict(critic=mk(hp["lr_critic"]), actor=mk(hp["lr_actor"])), gerr={})


def series_step(state, P_pre, grads, hp, variant=None):
    """One update of the series: P_pre the pre-update weights in float64, grads = series_grads at them.  Both optimisers step on
    every update with one step count; each target follows its stepped network.  -> (predicted tensors, bounds) over the four
    networks: Adam64's step at td3_f64.adam_step_bound (gerr the running maximum of the gradient bounds), the targets at
    soft_bound + tau x the step bound."""
    tau = hp["tau"]
    state["t"] += 1
    pred, bound = {}, {}
    for net in LOCAL:
        o = state["opt"][net]
        o.t = state["t"]
        o.lr = hp["lr_critic"] if variant == "one_lr" else hp["lr_" + net]
        o.b1, o.b2 = (hp["beta2"], hp["beta1"]) if variant == "betas_exchanged" else (hp["beta1"], hp["beta2"])
        if variant == "moments_not_carried":
            o.m.clear(); o.v.clear()
        tg = TARGET_OF[net]
        pred[net], bound[net], pred[tg], bound[tg] = {}, {}, {}, {}
        for k in R.NAMES:
            gb = grads[net]["bound"][k]
            ge = state["gerr"][(net, k)] = torch.maximum(state["gerr"].get((net, k), torch.zeros_like(gb)), gb)
            w1, ratio = o.step(k, P_pre[net][k], grads[net]["g"][k], t=1 if variant == "frozen_bias_correction" else None)
            sb = R.adam_step_bound(w1, ratio, o.lr, hp["eps"], ge)
            pred[net][k], bound[net][k] = w1, sb
            src = P_pre[net][k] if variant == "target_from_pre_step_weights" else w1
            pred[tg][k], bound[tg][k] = R.soft_update(P_pre[tg][k], src, tau), R.soft_bound(P_pre[tg][k], src, tau) + tau * sb
    return pred, bound


def series_ratios(got, pred, bound):
    return {(n, k): R.worst_ratio(got[n][k], pred[n][k], bound[n][k]) for n in pred for k in pred[n]}


def _net_worst(ratios, net):
    return max(v for (n, _), v in ratios.items() if n == net)


class EmulatedLearner:
    """The stand-in for the device handle in the CPU checks: float64 gradients rounded to float32 into td3_f64.adam_f32_emulation
    with carried moments and one step count, the soft updates in float32."""

    def __init__(self, P, shape, hp, cfg=SERIES_CFG):
        self.P = {n: {k: v.detach().clone().float() for k, v in p.items()} for n, p in P.items()}
        self.hp, self.cfg, self.t, self.mom, self.N = hp, cfg, 0, {}, R.chain_length(*shape)

    def update(self, batch):
        hp, f = self.hp, np.float32
        g = series_grads(R.to64(self.P), R.batch_double(batch), self.cfg, self.N)
        self.t += 1
        tau = f(hp["tau"])
        for net in LOCAL:
            for k in R.NAMES:
                m0, v0 = self.mom.get((net, k), (None, None))
                w1, m, v = R.adam_f32_emulation(self.P[net][k].numpy(), g[net]["g"][k].float().numpy(), hp["lr_" + net], hp["eps"], hp["beta1"],
                                                hp["beta2"], m0, v0, self.t)
                self.mom[(net, k)] = (m, v)
                self.P[net][k].copy_(torch.from_numpy(w1))
                tg = self.P[TARGET_OF[net]][k]
                tg.copy_(torch.from_numpy((tg.numpy() * (f(1) - tau) + w1 * tau).astype(f)))

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


def _dead_slices(p, dead):
    u1, u2 = dead
    return [p["w1"][u1], p["b1"][u1], p["w2"][:, u1], p["w2"][u2], p["b2"][u2], p["w3"][:, u2]]


def series_run(make_learner, shape, betas, device="cpu", cfg=SERIES_CFG, log=print):
    """SERIES_UPDATES updates of `make_learner(P, shape, hp)` (.P: its own float32 tensors on `device`, stepped in place;
    update(batch); close()) beside the float64 series, the margins re-established in place on the learner's tensors before every
    update after the first (only the hidden biases move); then a NEW learner on the stepped parameters for one more update.
    Asserts per update: no ambiguous ReLU mask; eps >= every gradient element; every tensor of the four networks within the
    series' bound; every wrong variant of SERIES_RULES rejected on each network it concerns from the update at which it can
    differ; the planted dead units' weights bit for bit.  -> dict(worst={net: ratio}, rejected={variant: smallest rejecting ratio})."""
    tag = "%s betas %.3g/%.4g" % ("x".join(map(str, shape)), betas[0], betas[1])
    P, batch, N, dead = series_case(shape, device, cfg)
    b64 = R.batch_double(batch)
    grads = series_grads(R.to64(P), b64, cfg, N)
    hp = series_hp(grads, betas, cfg["tau"])
    assert hp["lr_critic"] != hp["lr_actor"]
    log("%s: lr critic %g actor %g, eps %g" % (tag, hp["lr_critic"], hp["lr_actor"], hp["eps"]))
    right, wrong = series_state(hp), {v: series_state(hp) for v in SERIES_VARIANTS}
    worst, rejected = {}, {}
    zeros0 = [x.clone() for n in LOCAL for x in _dead_slices(P[n], dead[n])]
    be = make_learner(P, shape, hp)
    try:
        for u in range(SERIES_UPDATES + 1):
            if u == SERIES_UPDATES:                            # fresh state at create: a new learner on the stepped parameters
                stepped = {n: {k: v.clone() for k, v in p.items()} for n, p in be.P.items()}
                be.close()
                be = make_learner(stepped, shape, hp)
            if u:
                establish_margins(be.P, batch, cfg, N, rescale=False)
                grads = series_grads(R.to64(be.P), b64, cfg, N)
            assert margin_report(be.P, batch, cfg, N) >= 1.0, (tag, u, "margins")
            pre = {n: {k: v.clone() for k, v in p.items()} for n, p in R.to64(be.P).items()}
            top = max(float(v.abs().max()) for n in LOCAL for v in grads[n]["g"].values())
            assert top <= hp["eps"], (tag, u, "eps %g below the largest gradient element %g" % (hp["eps"], top))
            be.update(batch)
            got = R.to64(be.P)
            z_ = [x for n in LOCAL for x in _dead_slices(be.P[n], dead[n])]
            assert all(torch.equal(a_, b_) for a_, b_ in zip(z_, zeros0)), (tag, u, "a dead unit's weight moved")
            if u == SERIES_UPDATES:
                fresh = series_ratios(got, *series_step(series_state(hp), pre, grads, hp))
                carried = series_ratios(got, *series_step(right, pre, grads, hp))
                log("%s: new handle: fresh Adam %.3g, the carried one %s" % (tag, max(fresh.values()), {n: "%.3g" % _net_worst(carried, n) for n in LOCAL}))
                assert max(fresh.values()) <= 1.0, (tag, "fresh state at create", fresh)
                for n in LOCAL:
                    assert _net_worst(carried, n) > 1.0, (tag, "carried state accepted after create", n)
                    rejected["carried_after_create"] = min(rejected.get("carried_after_create", math.inf), _net_worst(carried, n))
                break
            ratios = series_ratios(got, *series_step(right, pre, grads, hp))
            for n in NETS:
                worst[n] = max(worst.get(n, 0.0), _net_worst(ratios, n))
            log("%s: update %d worst/bound %s" % (tag, u, {n: "%.3g" % _net_worst(ratios, n) for n in NETS}))
            assert max(ratios.values()) <= 1.0, (tag, u, {k: v for k, v in ratios.items() if v > 1.0})
            for var in SERIES_VARIANTS:
                rv = series_ratios(got, *series_step(wrong[var], pre, grads, hp, variant=var))
                first, nets = SERIES_RULES[var]
                if u < first:
                    continue
                per = {n: _net_worst(rv, n) for n in nets}
                log("%s: update %d %s %s" % (tag, u, var, {n: "%.3g" % v for n, v in per.items()}))
                for n, v in per.items():
                    assert v > 1.0, (tag, u, var, n, v)
                    rejected[var] = min(rejected.get(var, math.inf), v)
    finally:
        be.close()
    return dict(worst=worst, rejected=rejected, hp=hp)
