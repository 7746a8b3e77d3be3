"""tests/sac_f64.py against torch.autograd in float64 on the reference's loss expressions (sac.py:253-272), its statement of
cn_sac_act against crowdnav.sac.Agent.act in float64, the promises of act_case and box_muller_draw, and the series of four
updates: against crowdnav.sac.Agent.learn in float64 (torch.optim.Adam), and its acceptance rule's power on every case the GPU
tests run.  CPU only."""
import math

import numpy as np
import pytest
import torch

import adam_series as A
import sac_f64 as S
import td3_f64 as R
from actor_f64 import mix64, uniforms
from replay_distinct_ref import _mix_int
from sampling_f64 import noise_hash


def _autograd(P, batch, eps, variant=None):
    """sac.py's expressions with the head outputs as leaves: d policy_loss / d (mean, raw log_std), d q_loss / dQ, d value_loss / dV."""
    s, a, r, s2, d = batch
    c = S.CFG
    mean0, raw0, _, _ = S.trunk(P["actor"], s)
    mean, raw = mean0.detach().requires_grad_(True), raw0.detach().requires_grad_(True)
    ls = torch.clamp(raw, c["ls_min"], c["ls_max"])
    normal = torch.distributions.Normal(mean, ls.exp())
    z = (eps * ls.exp() + mean).detach()                        # .sample(): a value
    t = torch.tanh(z)
    logp = (normal.log_prob(z) - torch.log(1 - t.pow(2) + c["logp_eps"])).sum(-1, keepdim=True)
    a_new = torch.stack([torch.sigmoid(t[:, 0]) * c["max_v"], torch.tanh(t[:, 1]) * c["max_w"]], 1)
    q = S.mlp(P["q"], torch.cat([s, a], 1))[0].reshape(-1, 1).detach().requires_grad_(True)
    v = S.mlp(P["v"], s)[0].reshape(-1, 1).detach().requires_grad_(True)
    vt = S.mlp(P["v_t"], s2)[0].reshape(-1, 1)
    qn = S.mlp(P["q"], torch.cat([s, a_new], 1))[0].reshape(-1, 1)
    lq = torch.nn.functional.mse_loss(q, (r[:, None] + (1 - d[:, None]) * c["gamma"] * vt).detach())
    lv = torch.nn.functional.mse_loss(v, (qn - logp).detach())
    lp = (logp * (logp - (qn - v)).detach()).mean() + c["mean_lambda"] * mean.pow(2).mean() + c["std_lambda"] * ls.pow(2).mean() \
        + c["z_lambda"] * z.pow(2).sum(1).mean()
    gm, gr = torch.autograd.grad(lp, (mean, raw))
    (dq,) = torch.autograd.grad(lq, q)
    (dv,) = torch.autograd.grad(lv, v)
    return dict(dl=torch.cat([gm, gr], 1), dq=dq.reshape(-1), dv=dv.reshape(-1), loss=torch.stack([lq, lv, lp]).detach(), logp=logp.detach().reshape(-1))


@pytest.mark.parametrize("shape", [(20, 16, 2, 24), (13, 33, 17, 40), (9, 8, 1, 3)])
def test_formulas_equal_autograd_and_cover_the_clamp(shape):
    P, batch, eps, eps1, chain = S.make_case(*shape)
    P64, b64 = S.to64(P), tuple(x.double() for x in batch)
    R_ = S.rows(P64, b64, eps.double())
    A = _autograd(P64, b64, eps.double())
    for k in ("dl", "dq", "dv", "loss", "logp"):
        torch.testing.assert_close(R_[k], A[k], rtol=1e-9, atol=1e-12)
    raw = R_["raw"]
    assert bool((raw < -20).any()) and bool((raw > 2).any()) and bool(R_["inside"].bool().any())
    g_ls = R_["dl"][:, 2:]
    assert bool((g_ls[R_["inside"] == 0] == 0).all()) and bool((g_ls[R_["inside"] == 1] != 0).all())
    assert S.margins_ok(P64, b64, eps.double(), chain, S.clamp_chain(shape[0], shape[1]))
    assert float(S.clamp_margin(P64, b64, S.clamp_chain(shape[0], shape[1])).min()) > 1.0        # every element, no exception


def _weight_grads(P, batch, eps):
    """autograd through the three networks on sac.py's losses: {(net, name): gradient}."""
    s, a, r, s2, d = batch
    c = S.CFG
    L = {n: {k: v.detach().clone().requires_grad_(True) for k, v in P[n].items()} for n in ("actor", "q", "v")}
    mean, raw, _, _ = S.trunk(L["actor"], s)
    ls = torch.clamp(raw, c["ls_min"], c["ls_max"])
    z = (eps * ls.exp() + mean).detach()
    t = torch.tanh(z)
    logp = (torch.distributions.Normal(mean, ls.exp()).log_prob(z) - torch.log(1 - t.pow(2) + c["logp_eps"])).sum(-1)
    a_new = torch.stack([torch.sigmoid(t[:, 0]) * c["max_v"], torch.tanh(t[:, 1]) * c["max_w"]], 1)
    q, v = S.mlp(L["q"], torch.cat([s, a], 1))[0], S.mlp(L["v"], s)[0]
    vt, qn = S.mlp(P["v_t"], s2)[0], S.mlp(L["q"], torch.cat([s, a_new], 1))[0]
    lq = ((q - (r + (1 - d) * c["gamma"] * vt).detach()) ** 2).mean()
    lv = ((v - (qn - logp).detach()) ** 2).mean()
    lp = (logp * (logp - (qn - v)).detach()).mean() + c["mean_lambda"] * mean.pow(2).mean() + c["std_lambda"] * ls.pow(2).mean()
    out = {}
    for n, loss in (("q", lq), ("v", lv), ("actor", lp)):
        gs = torch.autograd.grad(loss, list(L[n].values()), retain_graph=True)
        out.update({(n, k): g for k, g in zip(L[n], gs)})
    return out


@pytest.mark.parametrize("shape", [(20, 16, 2, 24), (13, 33, 17, 40)])
def test_the_pass_equals_the_formulas_and_autograd_and_bounds_the_float32_update(shape):
    """run()'s exact pass: the rows' quantities equal rows(), every weight gradient equals autograd through the networks.  Its
    bounds hold the SAME pass evaluated in float32 on the CPU, and reject each quantity scaled by 1 + 1e-3."""
    P, batch, eps, eps1, chain = S.make_case(*shape)
    P64, b64 = S.to64(P), tuple(x.double() for x in batch)
    want, Bd = S.reference(P64, b64, eps.double())
    R_ = S.rows(P64, b64, eps.double())
    for k in S.KEYS + ("logp", "qn", "z"):
        torch.testing.assert_close(want[k], R_[k], rtol=1e-9, atol=1e-12)
    A = _weight_grads(P64, b64, eps.double())
    for k in S.GRADS:
        torch.testing.assert_close(want[k], A[k], rtol=1e-9, atol=1e-13)
        assert bool((want[k] != 0).any()), k
    f32 = S.run(R._Pass(), P, batch, eps)
    for k in S.KEYS + S.GRADS:
        assert R.worst_ratio(f32[k], want[k], Bd[k]) <= 1.0, k
    for k in ("dl", "dq", "dv"):
        assert R.worst_ratio(f32[k].double() * (1 + 1e-3), want[k], Bd[k]) > 1.0, k
    for i in range(3):
        assert float((f32["loss"][i].double() * (1 + 1e-3) - want["loss"][i]).abs() / Bd["loss"][i]) > 1.0, i
    for n in ("q", "v", "actor"):
        assert max(R.worst_ratio(f32[k].double() * (1 + 1e-3), want[k], Bd[k]) for k in S.GRADS if k[0] == n) > 1.0, n
    g_ls = f32["dl"][:, 2:]
    assert bool((g_ls[R_["inside"] == 0] == 0).all()) and bool((g_ls[R_["inside"] == 1] != 0).all())


def test_every_wrong_variant_differs_by_more_than_the_bounds():
    P, batch, eps, eps1, chain = S.make_case(20, 16, 2, 24)
    P64, b64 = S.to64(P), tuple(x.double() for x in batch)
    want, Bd = S.reference(P64, b64, eps.double())
    for var in S.VARIANTS[:4]:
        W = S.rows(P64, b64, eps.double(), variant=var, eps_first=eps1.double())
        Wp, _ = S.reference(P64, b64, eps.double(), variant=var, eps_first=eps1.double())
        for k in S.KEYS:
            torch.testing.assert_close(Wp[k], W[k], rtol=1e-9, atol=1e-12)
        worst = max(R.worst_ratio(Wp[k], want[k], Bd[k]) for k in S.KEYS + S.GRADS)
        assert worst > 1.0, (var, worst)
    assert all(bool(torch.isfinite(v).all()) for v in Bd.values())
    assert math.isfinite(float(want["loss"].sum()))


# ---- cn_sac_act's statement ---------------------------------------------------------------------------------------------------
def _agent64(pa, obs_dim, hidden):
    """crowdnav.sac.Agent on the CPU with its actor in float64 holding pa."""
    from crowdnav.sac import Agent
    ag = Agent(obs_dim=obs_dim, hidden=hidden, device="cpu", memory_size=4)
    ag.actor.double()
    a = ag.actor
    with torch.no_grad():
        for k, t in zip(S.ACTOR_NAMES, (a.linear1.weight, a.linear1.bias, a.linear2.weight, a.linear2.bias, a.mean_linear.weight,
                                        a.mean_linear.bias, a.log_std_linear.weight, a.log_std_linear.bias)):
            t.copy_(pa[k].double())
    return ag


@pytest.mark.parametrize("shape", [(17, 20, 24), (33, 13, 40), (1, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_act_pass_equals_agent_act_in_float64(shape):
    """act_pass with the exact _Pass() against Agent.act (actor.double()), sampled with supplied eps and deterministic: the twist
    to 1e-12, and mean / log_std / z against the actor's own forward."""
    H, D, n = shape
    pa, obs, eps = S.act_case(H, D, D + 3, n)
    ag = _agent64(pa, D, H)
    p64 = {k: v.double() for k, v in pa.items()}
    x, e = obs[:, :D].double(), eps.double()
    mean, ls, _ = ag.actor(x)
    for det in (False, True):
        got = S.act_pass(R._Pass(), p64, x, e, det)
        want = ag.act(obs.double(), eps=e, deterministic=det)
        assert want.dtype == torch.float64
        torch.testing.assert_close(got["twist"], want, rtol=0, atol=1e-12)
        torch.testing.assert_close(got["mean"], mean.detach(), rtol=0, atol=1e-12)
        torch.testing.assert_close(got["log_std"], ls.detach(), rtol=0, atol=1e-12)
        torch.testing.assert_close(got["z"], (mean if det else e * ls.exp() + mean).detach(), rtol=0, atol=1e-12)
        assert torch.equal(got["z"], got["mean"]) == det


def _check_case(H, D, n):
    pa, obs, eps = S.act_case(H, D, D + 3, n)
    assert obs.shape == (n, D + 3) and eps.shape == (n, 2) and bool(torch.isnan(obs[:, D:]).all()) and bool(torch.isfinite(obs[:, :D]).all())
    assert all(v.dtype == torch.float32 for v in pa.values()) and obs.dtype == torch.float32 and eps.dtype == torch.float32
    p64, x = {k: v.double() for k, v in pa.items()}, obs[:, :D].double()
    cc = S.clamp_chain(D, H)
    assert S.actor_margins_ok(p64, x, cc, cc), (H, D, n)                                   # every row: ReLU masks and clamp decisions
    assert float(S.clamp_margin({"actor": p64}, (x,), cc).min()) > 1.0, (H, D, n)
    below, inside, above = S.act_classes(pa, x)
    if S.act_promises_classes(H, n):
        assert bool(below.any()) and bool(inside.any()) and bool(above.any()), (H, D, n)
    raw = S.trunk(p64, x)[1]
    assert bool((eps[raw < S.EPS0_BELOW] == 0).all())
    assert bool(((eps.double() * raw.clamp(-20, 2).exp()).abs() <= S.Z_STEP_MAX * (1 + 1e-6)).all())
    again = S.act_case(H, D, D, n)
    assert torch.equal(again[1], obs[:, :D]) and torch.equal(again[2], eps) and all(torch.equal(again[0][k], pa[k]) for k in pa)
    return bool(below.any()), bool(above.any())


@pytest.mark.parametrize("H", S.ACT_HIDDEN)
def test_act_case_keeps_its_promises_at_every_shape_the_gpu_tests_use(H):
    """Margins on every row of every (hidden, D, n); the three clamp classes where hidden >= 15 and n >= 15; the same values
    whatever ld; eps zero below EPS0_BELOW and |eps| std <= Z_STEP_MAX."""
    for D in S.ACT_D:
        for n in S.ACT_N:
            _check_case(H, D, n)


def test_act_case_at_the_large_and_the_discrimination_shapes():
    for H, D, n in (S.ACT_LARGE,) + S.ACT_DISCRIMINATE:
        assert _check_case(H, D, n) == (True, True), (H, D, n)


@pytest.mark.parametrize("shape", S.ACT_DISCRIMINATE, ids=lambda s: "x".join(map(str, s)))
def test_every_wrong_act_variant_differs_by_more_than_twice_the_bound(shape):
    """Each ACT_VARIANTS entry, on the sampled path, moves some element of twist, z or log_std by more than twice the exact
    statement's propagated bound (the device may sit a bound away from float64 and must still be told apart), and the bounds hold
    the same pass evaluated in float32 on the CPU."""
    H, D, n = shape
    pa, obs, eps = S.act_case(H, D, D, n)
    p64, x, e = {k: v.double() for k, v in pa.items()}, obs.double(), eps.double()
    want, Bd = S.act_reference(p64, x, e, False)
    assert all(bool(torch.isfinite(v).all()) for v in Bd.values())
    for det in (False, True):
        w_, b_ = (want, Bd) if not det else S.act_reference(p64, x, e, True)
        f32 = S.act_pass(R._Pass(), pa, obs, eps, det)
        for k in S.ACT_KEYS:
            assert R.worst_ratio(f32[k], w_[k], b_[k]) <= 1.0, (k, det)
    for var in S.ACT_VARIANTS:
        wrong = S.act_pass(R._Pass(), p64, x, e, False, variant=var)
        worst = max(R.worst_ratio(wrong[k], want[k], 2 * Bd[k]) for k in ("twist", "z", "log_std"))
        assert worst > 1.0, (var, worst)


def test_mix64_is_splitmix64_and_the_same_on_ints_and_arrays():
    """splitmix64's first outputs from state 0 (Vigna's reference implementation) are mix64(0), mix64(0x9E3779B97F4A7C15), ...:
    of actor_f64.mix64, the one statement of cn_mix64, and of its form on Python ints, replay_distinct_ref._mix_int."""
    for mix in (_mix_int, lambda x: int(mix64(np.array([x], dtype=np.uint64))[0])):
        assert mix(0) == 0xE220A8397B1DCDAF and mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    xs = [0, 1, 7, (1 << 63) + 5, (1 << 64) - 1]
    assert mix64(np.array(xs, dtype=np.uint64)).tolist() == [_mix_int(x) for x in xs]


def test_box_muller_draw_keeps_what_the_device_draw_promises():
    """Over 2^20 rows: every u1 in (0, 1), u2 in [0, 1), each exactly a float32 value, every eps finite, mean and variance those
    of unit normals within 5 standard errors; rows and counters give different values.  The edges of the 24-bit integers: u1's
    smallest value is 2^-24 (r = 5.77), its largest -- at k = 2^24 - 1 alone, one hash in 2^24 -- is exactly 1, where r = 0 and
    eps = (0, 0): finite."""
    rows = np.arange(1 << 20)
    u1, u2 = uniforms(noise_hash(7, 3, None, rows))
    assert all(np.array_equal(u, u.astype(np.float32)) for u in (u1, u2))
    assert bool((u1 > 0).all()) and bool((u1 < 1).all()) and bool((u2 >= 0).all()) and bool((u2 < 1).all())
    e = S.box_muller_draw(7, 3, rows)
    assert e.shape == (1 << 20, 2) and bool(np.isfinite(e).all())
    k = e.size
    assert abs(float(e.mean())) <= 5 / math.sqrt(k) and abs(float(e.var()) - 1) <= 5 * math.sqrt(2.0 / k)
    assert len(np.unique(e.view(np.int64)[:, 0])) == 1 << 20
    assert not np.array_equal(e[:64], S.box_muller_draw(7, 4, rows[:64])) and not np.array_equal(e[:64], S.box_muller_draw(8, 3, rows[:64]))
    assert np.array_equal(S.box_muller_draw(7 + (1 << 64), 3, rows[:64]), e[:64])          # seed and counter are 64-bit
    edge = np.array([0, (1 << 64) - 1, ((1 << 24) - 1) << 40], dtype=np.uint64)
    eu1, eu2 = uniforms(edge)
    assert eu1.tolist() == [2.0 ** -24, 1.0, 1.0] and eu2.tolist() == [0.0, 1 - 2.0 ** -24, 0.0]
    h = noise_hash(0xD1B54A32D192ED03, (1 << 63) + 5, None, [0, 1, 4098])
    assert h.tolist() == [_mix_int(_mix_int(0xD1B54A32D192ED03 ^ _mix_int(((1 << 63) + 5) ^ 0x5bd1e995)) ^ m) for m in (0, 1, 4098)]


# ---- the series of four updates -----------------------------------------------------------------------------------------------
def _agent64_for_series(P, shape, hp):
    """crowdnav.sac.Agent on the CPU in float64 holding P, torch.optim.Adam at hp's betas / eps / lrs (value_net as written: width 2)."""
    from crowdnav.sac import Agent
    assert shape[2] == 2
    ag = Agent(obs_dim=shape[0], hidden=shape[1], actor_lr=hp["lr_actor"], v_lr=hp["lr_v"], q_lr=hp["lr_q"], batch_size=shape[3], memory_size=4,
               tau=hp["tau"], soft_update="intended" if hp["soft_update"] else "as_written", device="cpu")
    a = ag.actor
    mods = dict(actor=(a.linear1.weight, a.linear1.bias, a.linear2.weight, a.linear2.bias, a.mean_linear.weight, a.mean_linear.bias,
                       a.log_std_linear.weight, a.log_std_linear.bias))
    for n, m in (("q", ag.q), ("v", ag.v), ("v_t", ag.v_t)):
        mods[n] = (m.linear1.weight, m.linear1.bias, m.linear2.weight, m.linear2.bias, m.linear3.weight, m.linear3.bias)
    for m in (ag.actor, ag.q, ag.v, ag.v_t):
        m.double()
    with torch.no_grad():
        for n, ts in mods.items():
            for k, t in zip(S.ACTOR_NAMES if n == "actor" else S.NAMES, ts):
                t.copy_(P[n][k].double().reshape(t.shape))
    for o in (ag.opt_a, ag.opt_v, ag.opt_q):
        o.param_groups[0]["betas"], o.param_groups[0]["eps"] = (hp["beta1"], hp["beta2"]), hp["eps"]
    read = lambda: {n: {k: t.detach().clone().reshape(P[n][k].shape) for k, t in zip(S.ACTOR_NAMES if n == "actor" else S.NAMES, ts)} for n, ts in mods.items()}
    return ag, read


@pytest.mark.parametrize("soft_update", [0, 1])
def test_series_step_equals_agent_learn_in_float64(soft_update):
    """Four updates of sac.Agent.learn(batch=..., noise=...) cast to float64 (torch.optim.Adam; the product's betas) against
    series_step from the agent's own pre-update weights, a fresh eps each: every tensor within N 2^-53 (|w| + lr) -- the two
    differ by float64 rounding alone: N = chain_length roundings on the longest chain to a gradient element, each 2^-53 of its
    magnitude, and an element's step moves by lr x (its gradient's error) / eps <= lr x that, eps >= max |g|."""
    shape = (20, 16, 2, 24)
    P, batch, eps, _, chain = S.make_case(*shape)
    b64 = tuple(x.double() for x in batch)
    hp = S.series_hp(S.reference(S.to64(P), b64, eps.double())[0], S.SERIES_BETAS[1], soft_update)
    ag, read = _agent64_for_series(P, shape, hp)
    st = S.series_state(hp)
    gen = torch.Generator().manual_seed(9)
    worst = 0.0
    for u in range(4):
        e = eps.double() if u == 0 else torch.randn((shape[3], 2), generator=gen).double().clamp(-2, 2) * 0.1
        pre = read()
        ag.learn(batch=(b64[0], b64[1], b64[2][:, None], b64[3], b64[4][:, None]), noise=e)
        got = read()
        pred, _ = S.series_step(st, pre, b64, e, S.CFG, hp, ref=(S.run(R._Pass(), pre, b64, e), {k: torch.zeros(()) for k in S.GRADS}))
        for n in pred:
            lr = hp["lr_" + ("v" if n == "v_t" else n)]
            for k in pred[n]:
                tol = chain * 2.0 ** -53 * (pred[n][k].abs() + lr)
                worst = max(worst, float(((got[n][k] - pred[n][k]).abs() / tol).max()))
                assert bool(((got[n][k] - pred[n][k]).abs() <= tol).all()), (u, n, k)
                if u == 3 and not (n == "v_t" and soft_update == 0):
                    assert not torch.equal(got[n][k], P[n][k].double()), (n, k)
    print("soft_update %d: worst |agent - series| / (N 2^-53 (|w| + lr)) = %.3g" % (soft_update, worst))
    assert st["t"] == 4


@pytest.mark.parametrize("case", S.SERIES_CASES, ids=S.series_id)
def test_the_series_rule_accepts_a_float32_emulation_and_rejects_each_wrong_variant(case):
    """Every case of the GPU series test with the kernel's Adam formula emulated in float32 (td3_f64.adam_f32_emulation on
    float32-rounded float64 gradients, carried moments, one step count) in the handle's place: the inputs leave the emulation
    inside the series' bound at every update and every wrong variant outside it on each network it concerns, before anything
    runs on a GPU."""
    shape, betas, mode, clamp_all = case
    res = A.run(S.series(shape, betas, mode, clamp_all), S.EmulatedLearner, log=lambda s: None)
    print(S.series_id(case), {n: "%.3g" % v for n, v in res["worst"].items()}, {k: "%.3g" % v for k, v in res["rejected"].items()})
    assert max(res["worst"].values()) <= 1.0
    want = {v for v in S.SERIES_VARIANTS if mode in S.SERIES_RULES[v][0]} | {"carried_after_create"}
    assert set(res["rejected"]) == want and min(res["rejected"].values()) > 1.0
