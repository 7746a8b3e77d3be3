#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Golden vectors for the SAC learner (crowdnav.sac, cn_sac_update): the reference's own SAC classes
(turtlebot3_rl_sim/src/sac.py -- imports only torch / numpy, so it runs here unmodified) are imported from the reference tree
and driven on seeded inputs, with the arguments of sac.Agent in the order the class declares them:

  init.* / stepK.*   a small agent (46 -> 32 -> 32, batch 16, configs/sac.yaml's rates) built after torch.manual_seed(11): the
                     initial parameters of actor, v, v_t and q, and every parameter after each of four Agent.learn() calls on
                     one batch with random.sample pinned to the insertion order
  upd_*              that batch;  eps[K]: the unit normal behind the SECOND Normal.sample of call K (the one evaluate() uses;
                     forward() draws one before it and throws it away), recovered by redrawing torch.randn from the generator
                     state saved in front of the sample and checked here bit for bit: eps * std + mean == z
  loss[K]            (q, value, policy) of call K, recomputed beside it from the pre-call parameters on the same draws
  act_*              Agent.act() on a few observations: its eps, the clipped action

Writes tests/golden/sac.npz (data only).  Usage: python tools/make_sac_goldens.py [reference checkout]"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

REF_ROOT = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SRC = os.path.join(REF_ROOT, "turtlebot3_rl_sim", "src")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_sac", os.path.join(SRC, "sac.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.device = torch.device("cpu")
    return m


def flat(prefix, module, out):
    for k, v in module.state_dict().items():
        out["%s.%s" % (prefix, k)] = v.detach().cpu().numpy().copy()


def main():
    ref = load_ref()
    out = {}
    draws = []                                   # (eps, z) of every Normal.sample, in call order
    plain_sample = ref.Normal.sample

    def recording_sample(self, sample_shape=torch.Size()):
        state = torch.get_rng_state()
        z = plain_sample(self, sample_shape)
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        eps = torch.randn(z.shape)
        assert torch.equal(torch.get_rng_state(), after), "Normal.sample consumed the generator differently from torch.randn"
        assert torch.equal(eps * self.scale + self.loc, z), "Normal.sample is not randn * std + mean bit for bit"
        draws.append((eps.numpy().copy(), z.numpy().copy()))
        return z
    ref.Normal.sample = recording_sample

    H, B, D = 32, 16, 46
    torch.manual_seed(11)
    # sac.Agent's declared order: state, action, hidden, lr actor / v / q, batch, discount, buffer, tau, max_v, max_w, lambdas
    a = ref.Agent(D, 2, H, 3e-4, 3e-4, 3e-4, B, 0.99, 1000, 5e-3, 0.22, 2.0, 1e-3, 1e-3, 0.0)
    out["init_seed"] = np.int64(11)
    nets = dict(actor=a.actor, v=a.critic_v_net, v_t=a.critic_target_v_net, q=a.critic_soft_q_net)
    for k, m in nets.items():
        flat("init." + k, m, out)
    rng = np.random.RandomState(5)
    s = rng.uniform(-1, 1, (B, D)).astype(np.float32); s2 = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    ac = np.stack([rng.uniform(0, 0.22, B), rng.uniform(-2, 2, B)], 1).astype(np.float32)
    r = rng.uniform(-5, 5, B).astype(np.float32); d = (rng.uniform(0, 1, B) < 0.25)
    d[0], d[1] = False, True
    for i in range(B):
        a.memory.add(s[i], ac[i][None, :], float(r[i]), s2[i], bool(d[i]))    # the trainer stores action as (1, 2)
    out["upd_s"], out["upd_a"], out["upd_r"], out["upd_s2"], out["upd_d"] = s, ac, r, s2, d.astype(np.float32)
    ref.random.sample = lambda pop, k: list(pop)[:k]                          # pinned replay order
    st, at, rt, s2t, dt = [torch.from_numpy(x) for x in (s, ac, r[:, None], s2, d.astype(np.float32)[:, None])]
    losses, eps = [], []
    mse = torch.nn.functional.mse_loss
    for step in range(4):
        state = torch.get_rng_state()
        with torch.no_grad():                                               # learn()'s three losses (sac.py:253-272), recomputed
            qv, vv = a.critic_soft_q_net(st, at), a.critic_v_net(st)
            na, lp, z, mean, ls = a.actor.evaluate(st)
            lq = mse(qv, rt + (1 - dt) * 0.99 * a.critic_target_v_net(s2t))
            nq = a.critic_soft_q_net(st, na)
            lv = mse(vv, nq - lp)
            lpi = (lp * (lp - (nq - vv))).mean() + 1e-3 * mean.pow(2).mean() + 1e-3 * ls.pow(2).mean() + 0.0 * z.pow(2).sum(1).mean()
        losses.append([float(lq), float(lv), float(lpi)])
        torch.set_rng_state(state)
        del draws[:]
        a.learn()
        assert len(draws) == 2, "learn() draws two samples: forward()'s, then evaluate()'s"
        assert np.array_equal(draws[1][1], z.numpy())
        eps.append(draws[1][0])
        for k, m in nets.items():
            flat("step%d.%s" % (step, k), m, out)
    out["loss"] = np.array(losses, dtype=np.float32)
    out["eps"] = np.stack(eps).astype(np.float32)
    # ---- Agent.act ----
    obs = rng.uniform(-1, 1, (6, D)).astype(np.float32)
    acts, aeps = [], []
    for i in range(6):
        del draws[:]
        with contextlib.redirect_stdout(io.StringIO()):
            acts.append(np.asarray(a.act(obs[i]), dtype=np.float32)[0])
        assert len(draws) == 1
        aeps.append(draws[0][0][0])
    out["act_obs"], out["act_eps"], out["act_out"] = obs, np.stack(aeps).astype(np.float32), np.stack(acts)
    path = os.path.join(ROOT, "tests", "golden", "sac.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    # what the soft update of sac.py:290 moved (its arguments are (target, local) against soft_update(local, target))
    print("v_t moved over the four calls:", not np.array_equal(out["init.v_t.linear1.weight"], out["step3.v_t.linear1.weight"]))


if __name__ == "__main__":
    main()
