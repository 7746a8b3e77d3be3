"""tests/ddpg_f64.py's series of four updates on the CPU: against crowdnav.ddpg.Agent.learn in float64 (torch.optim.Adam), and
the power of its acceptance rule on every case the GPU test runs."""
import pytest
import torch

import adam_series as A
import ddpg_f64 as D
import td3_f64 as R


def _agent64(P, shape, hp):
    from crowdnav.ddpg import Agent
    ag = Agent(obs_dim=shape[0], hidden=shape[1], actor_lr=hp["lr_actor"], critic_lr=hp["lr_critic"], batch_size=shape[2], memory_size=4,
               tau=hp["tau"], device="cpu")
    mods = dict(actor=ag.actor, actor_t=ag.actor_t, critic=ag.critic, critic_t=ag.critic_t)
    ts = {n: (m.linear1.weight, m.linear1.bias, m.linear2.weight, m.linear2.bias, m.linear3.weight, m.linear3.bias) for n, m in mods.items()}
    for m in mods.values():
        m.double()
    with torch.no_grad():
        for n in ts:
            for k, t in zip(R.NAMES, ts[n]):
                t.copy_(P[n][k].double())
    for o in (ag.opt_a, ag.opt_c):
        o.param_groups[0]["betas"], o.param_groups[0]["eps"] = (hp["beta1"], hp["beta2"]), hp["eps"]
    return ag, lambda: {n: {k: t.detach().clone() for k, t in zip(R.NAMES, ts[n])} for n in ts}


def test_series_step_equals_agent_learn_in_float64():
    """Four updates of ddpg.Agent.learn(batch=...) cast to float64 (torch.optim.Adam; the product's betas) against series_step
    from the agent's own pre-update weights: every tensor within N 2^-53 (|w| + lr) -- float64 rounding alone: N = chain_length
    roundings on the longest chain to a gradient element, each 2^-53 of its magnitude; an element's step moves by
    lr x (its gradient's error) / eps <= lr x that, eps >= max |g|."""
    shape = (13, 24, 20)
    cfg = D.SERIES_CFG
    P, batch, N, _ = D.series_case(shape)
    b64 = R.batch_double(batch)
    hp = D.series_hp(D.series_grads(R.to64(P), b64, cfg, N), D.SERIES_BETAS[1], cfg["tau"])
    ag, read = _agent64(P, shape, hp)
    st = D.series_state(hp)
    worst = 0.0
    for u in range(4):
        pre = read()
        ag.learn(batch=(b64[0], b64[1], b64[2][:, None], b64[3], b64[4][:, None]))
        got = read()
        pred, _ = D.series_step(st, pre, D.series_grads(pre, b64, cfg, N), hp)
        for n in pred:
            lr = hp["lr_" + n.replace("_t", "")]
            for k in pred[n]:
                tol = N * 2.0 ** -53 * (pred[n][k].abs() + lr)
                worst = max(worst, float(((got[n][k] - pred[n][k]).abs() / tol).max()))
                assert bool(((got[n][k] - pred[n][k]).abs() <= tol).all()), (u, n, k)
    print("worst |agent - series| / (N 2^-53 (|w| + lr)) = %.3g" % worst)
    assert st["t"] == 4 and all(not torch.equal(got[n][k], P[n][k].double()) for n in ("actor", "critic") for k in ("w1", "w2", "w3"))


@pytest.mark.parametrize("case", D.SERIES_CASES, ids=D.series_id)
def test_the_series_rule_accepts_a_float32_emulation_and_rejects_each_wrong_variant(case):
    """Every case of the GPU series test with the kernel's Adam formula emulated in float32 (td3_f64.adam_f32_emulation on
    float32-rounded float64 gradients, carried moments, one step count) in the handle's place: inside the series' bound at every
    update, every wrong variant outside it on each network it concerns."""
    shape, betas = case
    res = A.run(D.series(shape, betas), D.EmulatedLearner, log=lambda s: None)
    print(D.series_id(case), {n: "%.3g" % v for n, v in res["worst"].items()}, {k: "%.3g" % v for k, v in res["rejected"].items()})
    assert max(res["worst"].values()) <= 1.0
    assert set(res["rejected"]) == set(D.SERIES_VARIANTS) | {"carried_after_create"} and min(res["rejected"].values()) > 1.0
