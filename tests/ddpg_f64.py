"""A float64 statement of one DDPG update (crowdnav.ddpg.Agent._update, ddpg.py:198-243 of the reference) for the tests of
cn_ddpg_update, built from the generic pieces of td3_f64 (forward passes, head derivatives, the propagated rounding bounds,
ReLU margins, the invertible Adam step).  What is DDPG's own: one critic and one target critic, y = r + (1 - d) gamma
Q_t(s2, pi_t(s2)) without target-policy noise, and the actor's gradient through the PRE-update critic -- so both gradients of
one update are functions of the same parameters and one kernel call yields them together."""
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


def establish_margins(P, batch, cfg, N, logit_scale=8.0):
    """td3_f64.establish_margins for DDPG's rows: the actor on s, actor_t on s2, the critic on (s, a) and (s, pi(s)), critic_t on
    (s2, pi_t(s2)).  Both policies' logits scaled to +-logit_scale first.  Modifies P's float32 tensors in place."""
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
