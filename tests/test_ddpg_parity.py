"""crowdnav.ddpg against golden vectors produced by the reference's own DDPG classes (tools/make_ddpg_goldens.py imports
turtlebot3_rl_sim/src/ddpg.py unmodified).  CPU-only: plain PyTorch modules, and the cn_ddpg_config ctypes layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ddpg.npz"))
NETS = ("actor", "actor_t", "critic", "critic_t")


def _agent(**kw):
    from crowdnav.ddpg import Agent
    return Agent(device="cpu", memory_size=64, **kw)


def _nets(ag):
    return dict(actor=ag.actor, actor_t=ag.actor_t, critic=ag.critic, critic_t=ag.critic_t)


def _load(ag, prefix):
    nets = _nets(ag)
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(G["%s.%s.%s" % (prefix, k, n)]) for n in m.state_dict()})
    return nets


def _batch():
    return (torch.from_numpy(G["upd_s"]), torch.from_numpy(G["upd_a"]), torch.from_numpy(G["upd_r"])[:, None],
            torch.from_numpy(G["upd_s2"]), torch.from_numpy(G["upd_d"])[:, None])


def test_seeded_initialisation_is_the_references():
    """Agent(seed) draws the reference's parameters: nn.Linear defaults, then linear3 of each network from U(-3e-3, 3e-3)
    (DDPG:75-76, 102-103) in DDPG:131-143's construction order, and the targets as hard copies (DDPG:150-151)."""
    ag = _agent(obs_dim=46, hidden=32, batch_size=16, seed=int(G["init_seed"]))
    for k, m in _nets(ag).items():
        for n, v in m.state_dict().items():
            assert np.array_equal(v.numpy(), G["init.%s.%s" % (k, n)]), (k, n)
    for a_, b_ in ((ag.actor, ag.actor_t), (ag.critic, ag.critic_t)):
        for x, y in zip(a_.parameters(), b_.parameters()):
            assert torch.equal(x, y)


def test_linear3_initialisation_range():
    ag = _agent(obs_dim=363, hidden=256, seed=3)
    with torch.no_grad():
        for m in (ag.actor, ag.critic):
            for p in (m.linear3.weight, m.linear3.bias):
                assert float(p.abs().max()) <= 3e-3                                    # U(-3e-3, 3e-3), not nn.Linear's 1/16
            assert float(m.linear3.weight.abs().max()) > 2.5e-3                        # (256 / 512 draws: the range is used)
            assert float(m.linear2.weight.abs().max()) > 0.05                          # the hidden layers keep the default


def test_four_updates_match_reference_learn():
    """Agent.learn (DDPG:198-243) with the replay order pinned: y from the single target critic, the actor step through the
    pre-update critic, the critic step, both soft updates (tau = 0.001).  Same tolerance as the TD3 parity test."""
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    nets = _load(ag, "init")
    batch = _batch()
    for step in range(4):
        loss = ag.learn(step, batch=batch)
        np.testing.assert_allclose(float(loss), float(G["loss"][step]), rtol=2e-5, atol=0)
        for k, m in nets.items():
            for n, v in m.state_dict().items():
                np.testing.assert_allclose(v.numpy(), G["step%d.%s.%s" % (step, k, n)], rtol=2e-5, atol=2e-7,
                                           err_msg="step %d %s.%s" % (step, k, n))
    # every update moves every network (no policy delay)
    for k in NETS:
        assert not np.array_equal(G["step0.%s.linear1.weight" % k], G["step1.%s.linear1.weight" % k]), k


def test_actor_step_uses_the_pre_update_critic():
    """The reference steps the actor before the critic (DDPG:233-239).  The order that steps the critic first (TD3's) gives
    an actor that does not match the golden; the right order does."""
    import torch.nn.functional as F
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    _load(ag, "init")
    s, a, r, s2, d = _batch()
    with torch.no_grad():
        y = r + (1.0 - d) * ag.gamma * ag.critic_t(s2, ag.actor_t(s2))
    lc = F.mse_loss(ag.critic(s, a), y)
    ag.opt_c.zero_grad(); lc.backward(); ag.opt_c.step()
    la = -ag.critic(s, ag.actor(s)).mean()
    ag.opt_a.zero_grad(); la.backward(); ag.opt_a.step()
    wrong = ag.actor.linear3.weight.detach().numpy()
    want = G["step0.actor.linear3.weight"]
    assert np.abs(wrong - want).max() > 100 * (2e-7 + 2e-5 * np.abs(want).max())


def test_hyper_parameters_are_the_reference_defaults():
    """TRAIN_DDPG:53-61 (batch 64, memory 1e6, 363 inputs, hidden 256, 0.22 / 2.0), configs/ddpg.yaml (actor 1e-4, critic 1e-3,
    gamma 0.99, tau 0.001), collection without exploration noise (TRAIN_DDPG:100), torch.optim.Adam's defaults."""
    import inspect
    from crowdnav.ddpg import Agent
    d = {k: v.default for k, v in inspect.signature(Agent.__init__).parameters.items() if v.default is not inspect._empty}
    assert d["batch_size"] == 64 and d["memory_size"] == 1_000_000 and d["hidden"] == 256 and d["obs_dim"] == 363
    assert d["actor_lr"] == 1e-4 and d["critic_lr"] == 1e-3 and d["gamma"] == 0.99 and d["tau"] == 0.001
    assert d["max_v"] == 0.22 and d["max_w"] == 2.0 and d["explore_sigma"] == 0.0
    ag = _agent(obs_dim=8, hidden=16)
    for o in (ag.opt_a, ag.opt_c):
        g = o.param_groups[0]
        assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 0 and not g["amsgrad"]


def test_ou_noise_is_the_references_on_a_pinned_stream():
    """OUNoise.sample (DDPG:56-64) driven by the same uniforms as the reference's random.random(), with the reset after the
    5th sample: x <- x + 0.15 (0 - x) + 0.2 U, float64."""
    from crowdnav.ddpg import OUNoise
    u = torch.from_numpy(G["ou_u"])
    ou = OUNoise(1)
    got = []
    for k in range(u.shape[0]):
        if k == int(G["ou_reset_at"]):
            ou.reset()
        got.append(ou.sample(k, u=u[k:k + 1])[0].numpy().copy())
    np.testing.assert_array_equal(np.stack(got), G["ou_x"])
    # one state per env, reset by mask
    ou = OUNoise(3)
    ou.sample(0, u=torch.ones((3, 2), dtype=torch.float64))
    ou.reset(torch.tensor([False, True, False]))
    assert float(ou.state[1].abs().max()) == 0.0 and float(ou.state[0].min()) == 0.2


def test_act_adds_ou_noise_only_when_asked_and_clips():
    ag = _agent(obs_dim=10, hidden=16, n_envs=4)
    obs = torch.randn(4, 10)
    a0 = ag.act(obs)
    assert torch.equal(a0, ag.act(obs)) and float(ag.noise.state.abs().max()) == 0.0
    a1 = ag.act(obs, add_noise=True)
    want = torch.max(torch.min((ag.actor(obs).double() + ag.noise.state).float(), ag._hi), ag._lo)
    assert torch.equal(a1, want.detach()) and not torch.equal(a0, a1)
    assert (a1[:, 0] >= 0).all() and (a1[:, 0] <= 0.22).all() and (a1[:, 1].abs() <= 2.0).all()
    ag.reset_noise(torch.tensor([True, True, True, True]))
    assert float(ag.noise.state.abs().max()) == 0.0


def test_checkpoints_save_the_targets_under_the_reference_names(tmp_path):
    """DDPG:262-272: the TARGET networks saved as ddpg_{actor,critic}_model_ep<N>.pt; load_models loads the locals and
    hard-copies the targets."""
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    _load(ag, "step3")                    # targets differ from the locals here
    assert not torch.equal(ag.actor.linear1.weight, ag.actor_t.linear1.weight)
    ag.save(str(tmp_path), 1500)
    names = sorted(os.listdir(tmp_path))
    assert names == ["ddpg_actor_model_ep1500.pt", "ddpg_critic_model_ep1500.pt"]
    sd = torch.load(os.path.join(tmp_path, names[0]))
    assert list(sd.keys()) == ["linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "linear3.weight", "linear3.bias"]
    other = _agent(obs_dim=46, hidden=32, seed=9)
    other.load_models(*[os.path.join(tmp_path, n) for n in names])
    for a_, b_ in ((ag.actor_t, other.actor), (ag.actor_t, other.actor_t), (ag.critic_t, other.critic), (ag.critic_t, other.critic_t)):
        for x, y in zip(a_.parameters(), b_.parameters()):
            assert torch.equal(x, y)


def test_shipped_checkpoints_load_strictly(tmp_path):
    """The key / shape table of the four shipped DDPG checkpoints (models/ddpg/trajectory_test, obs_layout 1: 363 inputs)
    loads with strict key matching into Actor(363) / Critic(363), through torch.save / load_models."""
    from crowdnav.td3 import Actor, Critic
    g = torch.Generator().manual_seed(0)
    sds = []
    for i, name in enumerate(G["ckpt_names"]):
        sd = {str(k): torch.rand([int(x) for x in shape if x >= 0], generator=g) - 0.5
              for k, shape in zip(G["ckpt%d_keys" % i], G["ckpt%d_shapes" % i])}
        m = Actor(363, 2, 256) if "actor" in str(name) else Critic(363, 2, 256)
        m.load_state_dict(sd, strict=True)
        torch.save(sd, tmp_path / str(name))
        sds.append(sd)
    ag = _agent(obs_dim=363, hidden=256)
    ag.load_models(str(tmp_path / str(G["ckpt_names"][2])), str(tmp_path / str(G["ckpt_names"][3])))
    assert torch.equal(ag.actor_t.linear1.weight, sds[2]["linear1.weight"]) and torch.equal(ag.critic.linear3.bias, sds[3]["linear3.bias"])
    # the recorded actions of the shipped ep3000 actor are actions (within the heads' ranges)
    act = G["shipped_act"]
    assert act.shape == (8, 2) and (act[:, 0] >= 0).all() and (act[:, 0] <= 0.22).all() and (np.abs(act[:, 1]) <= 2.0).all()


def test_ddpg_config_ctypes_layout_matches_the_header(tmp_path):
    """cn_ddpg_config: sizeof and the offset of every field as gcc lays out include/crowdnav.h, against the ctypes mirror."""
    from crowdnav import _abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _abi.CnDdpgConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(cn_ddpg_config));']
    lines += ['printf("%s %%zu\\n", offsetof(cn_ddpg_config, %s));' % (f[0], f[0]) for f in cls._fields_]
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]
    assert len(cls._fields_) == 25


def test_ddpg_entry_points_are_exported():
    import crowdnav
    crowdnav.build()
    L = C.CDLL(crowdnav._abi.LIB_PATH)
    for s in ("cn_ddpg_create", "cn_ddpg_destroy", "cn_ddpg_update", "cn_ddpg_loss_dev"):
        assert hasattr(L, s) and s in crowdnav._abi.EXPORTS
