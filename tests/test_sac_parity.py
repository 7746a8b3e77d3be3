"""crowdnav.sac against the reference's own SAC classes (tests/golden/sac.npz, written by tools/make_sac_goldens.py).  CPU only."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "sac.npz"))
NETS = ("actor", "v", "v_t", "q")


def _agent(**kw):
    from crowdnav.sac import Agent
    return Agent(device="cpu", memory_size=64, **kw)


def _nets(ag):
    return dict(actor=ag.actor, v=ag.v, v_t=ag.v_t, q=ag.q)


def _load(ag, prefix):
    nets = _nets(ag)
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(G["%s.%s.%s" % (prefix, k, n)]) for n in m.state_dict()})
    return nets


def _batch():
    return (torch.from_numpy(G["upd_s"]), torch.from_numpy(G["upd_a"]), torch.from_numpy(G["upd_r"])[:, None],
            torch.from_numpy(G["upd_s2"]), torch.from_numpy(G["upd_d"])[:, None])


def test_seeded_initialisation_is_the_references():
    """Agent(seed) draws the reference's parameters in SAC:169-181's order (actor, V, V_t, Q), V_t a hard copy of V (SAC:191);
    the state-dict keys are the reference's."""
    ag = _agent(obs_dim=46, hidden=32, batch_size=16, seed=int(G["init_seed"]))
    for k, m in _nets(ag).items():
        assert set(m.state_dict()) == {n[len("init.%s." % k):] for n in G.files if n.startswith("init.%s." % k)}
        for n, v in m.state_dict().items():
            assert np.array_equal(v.numpy(), G["init.%s.%s" % (k, n)]), (k, n)
    assert set(ag.actor.state_dict()) == {"%s.%s" % (l, p) for l in ("linear1", "linear2", "mean_linear", "log_std_linear") for p in ("weight", "bias")}


def test_value_net_as_written_and_intended():
    """As written (SAC:175-176): hidden width 2, linear3 ~ U(-hidden, hidden); both actor heads within 3e-3."""
    ag = _agent(obs_dim=363, hidden=256, seed=3)
    assert ag.v.linear1.weight.shape == (2, 363) and ag.v.linear2.weight.shape == (2, 2) and ag.v.linear3.weight.shape == (1, 2)
    assert float(ag.v.linear3.weight.abs().max()) > 3e-3 and float(ag.v.linear3.weight.abs().max()) <= 256
    assert G["init.v.linear3.weight"].shape == (1, 2) and np.abs(G["init.v.linear3.weight"]).max() > 3e-3
    for m in (ag.actor.mean_linear, ag.actor.log_std_linear):
        assert float(m.weight.abs().max()) <= 3e-3 and float(m.bias.abs().max()) <= 3e-3
    it = _agent(obs_dim=363, hidden=256, seed=3, value_net="intended")
    assert it.v.linear2.weight.shape == (256, 256) and float(it.v.linear3.weight.abs().max()) <= 3e-3


def test_four_updates_match_reference_learn():
    """Agent.learn (SAC:231-290) on the pinned batch and the eps of its second Normal.sample; tolerances of the DDPG parity test."""
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    nets = _load(ag, "init")
    batch = _batch()
    for step in range(4):
        loss = ag.learn(step, batch=batch, noise=torch.from_numpy(G["eps"][step]))
        assert loss.shape == (3,)
        np.testing.assert_allclose(loss.numpy(), G["loss"][step], rtol=2e-5, atol=0)
        for k, m in nets.items():
            for n, v in m.state_dict().items():
                np.testing.assert_allclose(v.numpy(), G["step%d.%s.%s" % (step, k, n)], rtol=2e-5, atol=2e-7,
                                           err_msg="step %d %s.%s" % (step, k, n))


def test_soft_update_as_written_moves_v_not_its_target():
    """SAC:290 passes (V_t, V) to soft_update(local, target): the reference's V_t never moves (the goldens show it), V does."""
    for n in ("linear1.weight", "linear3.bias"):
        assert np.array_equal(G["init.v_t." + n], G["step3.v_t." + n])
        assert not np.array_equal(G["init.v." + n], G["step3.v." + n])
    ag = _agent(obs_dim=46, hidden=32, batch_size=16, soft_update="intended")
    _load(ag, "init")
    ag.learn(0, batch=_batch(), noise=torch.from_numpy(G["eps"][0]))
    assert not np.array_equal(ag.v_t.linear1.weight.detach().numpy(), G["init.v_t.linear1.weight"])


def test_learn_draws_twice_and_uses_the_second_sample():
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    _load(ag, "init")
    ag2 = _agent(obs_dim=46, hidden=32, batch_size=16)
    _load(ag2, "init")
    torch.manual_seed(5)
    l1 = ag.learn(0, batch=_batch())
    torch.manual_seed(5)
    torch.randn(16, 2)
    l2 = ag2.learn(0, batch=_batch(), noise=torch.randn(16, 2))
    assert torch.equal(l1, l2)


def test_act_matches_the_reference_with_its_eps():
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    _load(ag, "step3")
    a = ag.act(torch.from_numpy(G["act_obs"]), eps=torch.from_numpy(G["act_eps"]))
    np.testing.assert_allclose(a.numpy(), G["act_out"], rtol=2e-6, atol=1e-7)
    det = ag.act(torch.from_numpy(G["act_obs"]), deterministic=True)
    assert torch.equal(det, ag.act(torch.from_numpy(G["act_obs"]), deterministic=True))


def test_action_range_is_the_double_squash():
    ag = _agent(obs_dim=46, hidden=32, seed=1)
    obs = torch.randn(512, 46) * 3
    a = ag.act(obs, eps=torch.randn(512, 2) * 50)
    v = a[:, 0] / ag.max_v
    sig = lambda x: 1 / (1 + math.exp(-x))
    assert float(v.min()) >= sig(-1) - 1e-6 and float(v.max()) <= sig(1) + 1e-6
    assert float((a[:, 1] / ag.max_w).abs().max()) <= math.tanh(1) + 1e-6


def test_learn_waits_for_more_than_a_batch():
    ag = _agent(obs_dim=46, hidden=32, batch_size=16)
    s, a, r, s2, d = _batch()
    ag.memory.add(s, a, r, s2, d)
    assert ag.learn() is None
    ag.memory.add(s[:1], a[:1], r[:1], s2[:1], d[:1])
    assert ag.learn().shape == (3,)


def test_checkpoints_use_the_reference_names_and_v_holds_the_target(tmp_path):
    ag = _agent(obs_dim=46, hidden=32, batch_size=16, soft_update="intended")
    _load(ag, "init")
    ag.learn(0, batch=_batch(), noise=torch.from_numpy(G["eps"][0]))
    ag.save(str(tmp_path), 7)
    names = ["sac_actor_model_ep7.pt", "sac_critic_v_model_ep7.pt", "sac_critic_soft_q_model_ep7.pt"]
    assert sorted(os.listdir(tmp_path)) == sorted(names)
    sd = torch.load(tmp_path / names[1])
    assert torch.equal(sd["linear1.weight"], ag.v_t.linear1.weight) and not torch.equal(sd["linear1.weight"], ag.v.linear1.weight)
    other = _agent(obs_dim=46, hidden=32, batch_size=16, seed=9)
    other.load_models(*[str(tmp_path / n) for n in names])
    for m, o in ((ag.actor, other.actor), (ag.q, other.q), (ag.v_t, other.v), (ag.v_t, other.v_t)):
        for x, y in zip(m.parameters(), o.parameters()):
            assert torch.equal(x, y)


@pytest.mark.parametrize("name,struct", [("CnSacConfig", "cn_sac_config"), ("CnSacActIO", "cn_sac_act_io")])
def test_sac_ctypes_layout_matches_the_header(tmp_path, name, struct):
    from crowdnav import _abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = getattr(_abi, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %%zu\\n", sizeof(%s));' % struct]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], struct, f[0]) for f in cls._fields_]
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


def test_sac_entry_points_are_exported():
    import crowdnav
    crowdnav.build()
    L = C.CDLL(crowdnav._abi.LIB_PATH)
    for s in ("cn_sac_create", "cn_sac_destroy", "cn_sac_update", "cn_sac_loss_dev", "cn_sac_batch_dev", "cn_sac_act"):
        assert hasattr(L, s) and s in crowdnav._abi.EXPORTS


def test_trainer_knows_sac():
    from crowdnav import train
    a = train.parse_args(["--algo", "sac"])
    assert a.obs_layout == 1 and a.max_steps == 1000 and a.sac_value_net == "as-written" and a.out == "runs/sac"
    assert train.CHECKPOINT_NETS["sac"] == ("actor", "critic_v", "critic_soft_q")
