"""CPU checks of tests/td3_f64.py, the float64 reference and the comparison tools of tests/test_gpu_td3_f64.py: the Adam
inversion recovers a float32 gradient to the precision the GPU test assumes, the margin construction leaves no ambiguous ReLU
mask, and the tolerance accepts a float32 evaluation of the update while rejecting each plausible wrong variant of it."""
import copy

import numpy as np
import torch

import td3_f64 as R

CFG = dict(gamma=0.99, tau=2.0 ** -4, max_v=0.22, max_w=2.0, noise_std=0.25, noise_clip=0.5)


def _case(obs_dim=13, hidden=24, batch=20, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = R.new_params(obs_dim, hidden, g, dtype=torch.float32)
    s = (torch.randn((batch, obs_dim), generator=g) * 0.5).float()
    a = torch.stack([torch.rand(batch, generator=g) * 0.22, torch.rand(batch, generator=g) * 4 - 2], 1).float()
    r = (2 + 0.5 * torch.randn(batch, generator=g)).float()
    s2 = (torch.randn((batch, obs_dim), generator=g) * 0.5).float()
    d = (torch.rand(batch, generator=g) < 0.3).float()
    nz = torch.randn((batch, 2), generator=g).float()
    nz[0::5, 0] = 2.0; nz[1::5, 1] = -2.0; nz[2::7] = 10.0          # exactly +-noise_clip, and beyond it
    batch_ = (s, a, r, s2, d, nz)
    dead = R.plant_dead_units(P, hidden)
    N = R.chain_length(obs_dim, hidden, batch)
    R.establish_margins(P, batch_, CFG, N)
    return P, batch_, N, dead


def test_inverting_the_kernels_float32_adam_step_recovers_the_gradient():
    """beta1 = beta2 = 0: the kernel's formula in float32 (numpy emulation), then invert_step in float64.  The recovered g is
    within inversion_bound of the float32 g, and that bound is what the GPU test adds to its tolerance; the worst error is about
    1e-7 max|g| at w ~ 0.05, eps 4, lr 1024, as the bound's absolute term predicts.  g = 0 leaves w bit for bit."""
    rng = np.random.default_rng(0)
    n = 200000
    w = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g = (rng.uniform(-1, 1, n) * 4.0 * 10.0 ** rng.uniform(-8, 0, n)).astype(np.float32)
    g[:100] = 0
    g[100:200] = 4.0                                                 # |g| = eps: |u| = 1/2, the edge of the well-conditioned range
    for lr, eps in ((1024.0, 4.0), (1024.0, 2.0 ** -10), (2.0 ** 14, 1.0)):
        gg = np.clip(g, -eps, eps)
        w1, _, _ = R.adam_f32_emulation(w, gg, lr, eps)
        assert np.array_equal(w1[:100], w[:100])
        tw, tw1, tg = torch.from_numpy(w), torch.from_numpy(w1), torch.from_numpy(gg).double()
        rec = R.invert_step(tw, tw1, lr, eps)
        err = (rec - tg).abs()
        bnd = R.inversion_bound(tg, tw, tw1, lr, eps)
        assert bool((err <= bnd).all()), float((err / bnd).max())
        if lr == 1024.0 and eps == 4.0:
            assert float(err.max()) <= 2e-7 * float(tg.abs().max())


def test_margins_leave_no_pre_activation_within_its_rounding_bound():
    for shape in ((13, 24, 20), (1, 4, 3), (31, 17, 33), (5, 1, 9)):
        P, batch, N, dead = _case(*shape)
        worst, ndead, per = R.margin_report(P, batch, CFG, N)
        assert worst >= 1.0, (shape, worst, per)
        assert (ndead > 0) == (shape[1] >= 4)
    # without the construction, networks of the product's size do have ambiguous units (the check is not vacuous)
    g = torch.Generator().manual_seed(3)
    P = R.new_params(200, 256, g, dtype=torch.float32)
    s = torch.randn((128, 200), generator=g).float() * 0.5
    a = torch.rand((128, 2), generator=g).float()
    batch = (s, a, torch.ones(128), s, torch.zeros(128), torch.zeros((128, 2)))
    assert R.margin_report(P, batch, CFG, R.chain_length(200, 256, 128))[0] < 1.0


def test_min_of_the_target_critics_picks_both_sides_and_logits_reach_saturation():
    P, batch, N, _ = _case(13, 24, 40)
    t = R.td_target(R.to64(P), R.batch_double(batch), CFG)
    frac = float((t["q1t"] < t["q2t"]).double().mean())
    assert 0.2 <= frac <= 0.8
    lg = R.actor_fwd(R.to64(P)["actor"], batch[0].double(), CFG)["logits"]
    assert 7.0 <= float(lg.abs().max()) <= 9.0


def _f32_update(P, batch, lr_c, lr_a, b1, b2, eps, do_actor, optc, opta):
    """A float32 evaluation of the update in another summation order (PyTorch's), Adam emulated in float32: the stand-in for
    the kernel in these CPU checks."""
    N = 0
    c = R.critic_grads(P, batch, CFG)
    out = {n: {k: v.clone() for k, v in p.items()} for n, p in P.items()}
    for net in ("q1", "q2"):
        for k in R.NAMES:
            st = optc.setdefault((net, k), [None, None])
            w1, st[0], st[1] = R.adam_f32_emulation(P[net][k].numpy(), c[net]["g"][k].float().numpy(), lr_c, eps, b1, b2, st[0], st[1], optc["t"])
            out[net][k] = torch.from_numpy(w1)
    if do_actor:
        ag = R.actor_grads({**P, "q1": out["q1"]}, batch[0], CFG)
        for k in R.NAMES:
            st = opta.setdefault(k, [None, None])
            w1, st[0], st[1] = R.adam_f32_emulation(P["actor"][k].numpy(), ag["g"][k].float().numpy(), lr_a, eps, b1, b2, st[0], st[1], opta["t"])
            out["actor"][k] = torch.from_numpy(w1)
        for t, src in (("q1_t", "q1"), ("q2_t", "q2"), ("actor_t", "actor")):
            for k in R.NAMES:
                out[t][k] = (P[t][k] * (1 - CFG["tau"]) + out[src][k] * CFG["tau"]).float()
    return out


def test_the_tolerance_accepts_a_float32_update_and_rejects_each_wrong_variant():
    """Invertible Adam on a float32 (PyTorch-order) evaluation: the recovered gradients pass compare_grads; the gradient x
    (1 + 1e-3), one 16 x 16 tile zeroed, and y from Q1_t alone fail it.  Two updates with betas 0.5 / 0.75 (the actor on the
    second only, so its step count is 1 where the critics' is 2): the predicted weights pass adam_step_bound; the actor through the
    pre-update Q1, the actor's bias correction with the critics' step count, and the soft update from the pre-step weights fail."""
    P, batch, N, _ = _case(37, 40, 24)
    b64 = R.batch_double(batch)
    ref = R.critic_grads(R.to64(P), b64, CFG)
    eps = 2.0 ** np.ceil(np.log2(max(float(ref[n]["g"][k].abs().max()) for n in ("q1", "q2") for k in R.NAMES)))
    L = 1024.0
    got = _f32_update(P, batch, L, 0.0, 0.0, 0.0, eps, 0, {"t": 1}, {"t": 1})
    accept = lambda r: max(r.values()) <= 1.0
    for net in ("q1", "q2"):
        gk = {k: R.invert_step(P[net][k], got[net][k], L, eps) for k in R.NAMES}
        extra = {k: R.inversion_bound(gk[k], P[net][k], got[net][k], L, eps) for k in R.NAMES}
        assert accept(R.compare_grads(gk, ref[net]["g"], ref[net]["bound"], extra))
        scaled = {k: v * (1 + 1e-3) for k, v in ref[net]["g"].items()}
        assert not accept(R.compare_grads(gk, scaled, ref[net]["bound"], extra))
        tiled = dict(ref[net]["g"], w2=R.zero_tile(ref[net]["g"]["w2"]))
        assert not accept(R.compare_grads(gk, tiled, ref[net]["bound"], extra))
    cfg1 = dict(CFG, gamma=CFG["gamma"])
    wrong_y = R.critic_grads(R.to64(P), b64, cfg1, y_from="q1t")
    gk = {k: R.invert_step(P["q1"][k], got["q1"][k], L, eps) for k in R.NAMES}
    extra = {k: R.inversion_bound(gk[k], P["q1"][k], got["q1"][k], L, eps) for k in R.NAMES}
    assert not accept(R.compare_grads(gk, wrong_y["q1"]["g"], wrong_y["q1"]["bound"], extra))
    assert float(ref["t"]["y"].sub(wrong_y["t"]["y"]).abs().max()) > 0
    # Adam across two updates, the actor on the second
    lr, lra, b1, b2 = 2.0 ** -2, 2.0 ** -8, 0.5, 0.75      # the critics move far enough that "pre-update Q1" is visible
    optc, opta = {"t": 0}, {"t": 0}
    o64c = {n: R.Adam64(lr, b1, b2, eps) for n in ("q1", "q2")}
    o64a = R.Adam64(lra, b1, b2, eps)
    cur = P
    for step, do_actor in enumerate((0, 1)):
        optc["t"] += 1
        opta["t"] += do_actor
        pre = R.to64(cur)
        c = R.critic_grads(pre, b64, CFG)
        nxt = _f32_update(cur, batch, lr, lra, b1, b2, eps, do_actor, optc, opta)
        for n in ("q1", "q2"):
            o64c[n].t += 1
            for k in R.NAMES:
                w_pred, ratio = o64c[n].step(k, pre[n][k], c[n]["g"][k])
                assert R.worst_ratio(nxt[n][k], w_pred, R.adam_step_bound(w_pred, ratio, lr, eps, c[n]["bound"][k])) <= 1.0
        if do_actor:
            post_q1 = R.to64(nxt)["q1"]
            a_ok = R.actor_grads(pre, b64[0], CFG, q1=post_q1, N_mask=N)
            a_pre = R.actor_grads(pre, b64[0], CFG)
            o64a.t += 1
            variants = {"right": (a_ok, None), "pre-update Q1": (a_pre, None), "critic step count": (a_ok, o64c["q1"].t)}
            for name, (ag, t_override) in variants.items():
                o = copy.deepcopy(o64a)
                res = []
                for k in R.NAMES:
                    w_pred, ratio = o.step(k, pre["actor"][k], ag["g"][k], t=t_override)
                    res.append(R.worst_ratio(nxt["actor"][k], w_pred, R.adam_step_bound(w_pred, ratio, lra, eps, ag["bound"][k])))
                assert (max(res) <= 1.0) == (name == "right"), (name, res)
            for t, src in (("q1_t", "q1"), ("actor_t", "actor")):
                for k in R.NAMES:
                    right = R.soft_update(pre[t][k], nxt[src][k].double(), CFG["tau"])
                    wrong = R.soft_update(pre[t][k], pre[src][k], CFG["tau"])
                    bnd = R.soft_bound(pre[t][k], nxt[src][k].double(), CFG["tau"])
                    assert R.worst_ratio(nxt[t][k], right, bnd) <= 1.0
                    if k == "w2":
                        assert R.worst_ratio(nxt[t][k], wrong, bnd) > 1.0
        cur = nxt


def test_the_propagated_passes_hand_written_backward_equals_autograd():
    """propagated_bounds perturbs a hand-written forward / backward (_Pass); unperturbed it must be the autograd gradients."""
    P, batch, N, _ = _case(19, 33, 21)
    P64, b64 = R.to64(P), R.batch_double(batch)
    crit, _ = R.propagated_bounds(lambda ps: {(n, k): v for n, g in ps.critics(P64, b64, CFG).items() for k, v in g.items()}, samples=1)
    act, _ = R.propagated_bounds(lambda ps: ps.actor(P64, b64[0], CFG, P64["q1"]), samples=1)
    ref = R.critic_grads(P64, b64, CFG)
    refa = R.actor_grads(P64, b64[0], CFG)
    for k in R.NAMES:
        for n in ("q1", "q2"):
            torch.testing.assert_close(crit[(n, k)], ref[n]["g"][k], rtol=1e-10, atol=1e-14)
        torch.testing.assert_close(act[k], refa["g"][k], rtol=1e-10, atol=1e-14)


def test_the_bound_rejects_zero_and_scaled_gradients_at_the_product_shape():
    """The tolerance is narrow where it matters: at (398, 256, 128) the float32 PyTorch evaluation passes, while a zero
    gradient, x 2 and x (1 + 1e-3) fail, for the critics and the actor."""
    P, batch, N, _ = _case(398, 256, 128)
    P64, b64 = R.to64(P), R.batch_double(batch)
    ref = R.critic_grads(P64, b64, CFG)
    f32 = R.critic_grads(P, batch, CFG)
    refa = R.actor_grads(P64, b64[0], CFG)
    f32a = R.actor_grads(P, batch[0], CFG)
    accept = lambda got, r: max(R.compare_grads(got, r["g"], r["bound"]).values()) <= 1.0
    for r, got in ((ref["q1"], f32["q1"]["g"]), (ref["q2"], f32["q2"]["g"]), (refa, f32a["g"])):
        assert accept(got, r)
        for wrong in ({k: torch.zeros_like(v) for k, v in r["g"].items()}, {k: 2 * v for k, v in r["g"].items()},
                      {k: v * (1 + 1e-3) for k, v in r["g"].items()}):
            assert not accept(wrong, r)
