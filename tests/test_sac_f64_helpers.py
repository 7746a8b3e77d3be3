"""tests/sac_f64.py against torch.autograd in float64 on the reference's loss expressions (sac.py:253-272).  CPU only."""
import math

import pytest
import torch

import sac_f64 as S
import td3_f64 as R


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
