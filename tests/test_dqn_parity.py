"""crowdnav.dqn on the CPU: the epsilon schedule of the logged run, the reference's defaults and initialisation, the chunked
update (deepq.py:219-266 + Keras fit) against the float64 statement in tests/dqn_f64.py, checkpoints, and the ctypes layouts
of cn_dqn_config / cn_dqn_act_io against include/crowdnav.h."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dqn_f64 as Q
from conftest import ROOT


def _agent(**kw):
    from crowdnav.dqn import Agent
    kw.setdefault("memory_size", 64)
    return Agent(device="cpu", **kw)


def _params(net):
    return {k: getattr(getattr(net, "linear%d" % int(k[1])), "weight" if k[0] == "w" else "bias").detach().double().numpy()
            for k in ("w1", "b1", "w2", "b2", "w3", "b3")}


def test_epsilon_schedule_reaches_the_checkpoints_value():
    """1 500 applications of TRAIN_DQN:89-90 from 1.0: dqn_model_ep1500.json's explorationRate, bit for bit."""
    from crowdnav.dqn import epsilon_after
    assert epsilon_after(1500) == 0.049911691230058335
    ag = _agent(obs_dim=8, hidden=(16, 16))
    for _ in range(1500):
        ag.start_episode()
    assert ag.epsilon == 0.049911691230058335
    assert epsilon_after(10 ** 6) == epsilon_after(1500)      # stops once at or below 0.05
    assert epsilon_after(1, epsilon=0.0) == 0.0                # dqn.yaml's committed epsilon: 0.0 stays 0


def test_hyper_parameters_are_the_reference_defaults():
    import inspect
    from crowdnav.dqn import Agent
    d = {k: v.default for k, v in inspect.signature(Agent.__init__).parameters.items() if v.default is not inspect._empty}
    assert d["obs_dim"] == 361 and tuple(d["hidden"]) == (300, 300) and d["n_actions"] == 3
    assert d["batch_size"] == 64 and d["learn_start"] == 64 and d["memory_size"] == 1_000_000 and d["target_update"] == 10000
    assert d["gamma"] == 0.99 and d["lr"] == 2.5e-4 and d["rho"] == 0.9 and d["eps"] == 1e-6
    assert d["epsilon"] == 1.0 and d["epsilon_discount"] == 0.995 and d["epsilon_min"] == 0.05
    g = _agent(obs_dim=8, hidden=(16, 16)).opt.param_groups[0]
    assert g["alpha"] == 0.9 and g["eps"] == 1e-6 and g["momentum"] == 0 and not g["centered"] and g["weight_decay"] == 0


def test_lecun_uniform_initialisation():
    ag = _agent(obs_dim=361, hidden=(300, 300), seed=1)
    for m in (ag.q.linear1, ag.q.linear2, ag.q.linear3):
        lim = math.sqrt(3.0 / m.in_features)
        w = m.weight.detach()
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.95 * lim
        assert abs(float(w.std()) - lim / math.sqrt(3.0)) < 0.05 * lim
        assert float(m.bias.abs().max()) == 0.0
    for x, y in zip(ag.q.parameters(), ag.q_t.parameters()):
        assert torch.equal(x, y)


def _batch(B, ld, n_final, seed):
    g = torch.Generator().manual_seed(seed)
    s, s2 = torch.rand((B, ld), generator=g) * 3.5, torch.rand((B, ld), generator=g) * 3.5
    a = torch.randint(0, 3, (B,), generator=g)
    r = torch.randn(B, generator=g) * 10
    d = torch.zeros(B)
    d[torch.randperm(B, generator=g)[:n_final]] = 1.0
    return s, a, r, s2, d


@pytest.mark.parametrize("nf", [0, 1, 7])
def test_torch_learn_matches_the_f64_statement(nf):
    """The PyTorch update (the comparison path): X_batch / Y_batch in the reference's order, one step on the first 64 shuffled
    rows and a second on the F after them, RMSprop as Keras's."""
    D, ld, H, B = 30, 33, 40, 16
    ag = _agent(obs_dim=D, obs_ld=ld, hidden=(H, H), batch_size=B, lr=1e-2, seed=nf)
    batch = _batch(B, ld, nf, seed=10 + nf)
    p0 = _params(ag.q)
    acc = {k: np.zeros_like(v) for k, v in p0.items()}
    perm = np.random.default_rng(nf).permutation(B + nf)
    X, Y, src = ag.targets(*batch)
    nb = (batch[0][:, :D].double().numpy(), batch[1].numpy(), batch[2].double().numpy(), batch[3][:, :D].double().numpy(), batch[4].numpy() != 0)
    want, _, info = Q.update(p0, p0, acc, nb, perm, 0.99, 1e-2, 0.9, 1e-6, False)
    assert np.array_equal(src.numpy(), info["src"])
    np.testing.assert_allclose(X.double().numpy(), info["X"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(Y.double().numpy(), info["Y"], rtol=1e-5, atol=1e-4)
    ag.learn(batch=batch, perm=perm)
    got = _params(ag.q)
    for k in got:
        step = np.abs(want[k] - p0[k]).max()
        assert np.abs(got[k] - want[k]).max() <= 1e-3 * step, k
    if nf:                                                          # the two-chunk semantics is what the weights show
        one = Q.update(p0, p0, acc, nb, perm, 0.99, 1e-2, 0.9, 1e-6, False, variant="skip_chunk2")[0]
        assert max(np.abs(got[k] - one[k]).max() / np.abs(want[k] - p0[k]).max() for k in got) > 1e-2


def test_final_rows_follow_their_sample_and_carry_the_reward():
    ag = _agent(obs_dim=4, obs_ld=4, hidden=(8, 8), batch_size=4)
    s = torch.arange(16.0).reshape(4, 4); s2 = -s
    X, Y, src = ag.targets(s, torch.tensor([0, 1, 2, 0]), torch.tensor([1.0, 2.0, 3.0, 4.0]), s2, torch.tensor([0.0, 1.0, 0.0, 1.0]))
    assert src.tolist() == [0, 1, 5, 2, 3, 7]
    assert torch.equal(X[2], s2[1]) and torch.equal(Y[2], torch.full((3,), 2.0)) and torch.equal(Y[5], torch.full((3,), 4.0))
    assert float(Y[1, 1]) == 2.0 and float(Y[4, 0]) == 4.0          # a final sample's own row: Y[a] = r


def test_select_action_pinned_draws_and_twists():
    ag = _agent(obs_dim=6, hidden=(8, 8))
    obs = torch.rand(5, 6)
    greedy = torch.argmax(ag.q_values(obs), 1)
    u = torch.tensor([0.0, 0.5, 0.99, 0.2, 0.7], dtype=torch.float64)
    pick = torch.tensor([2, 2, 2, 1, 0])
    got = ag.select(obs, epsilon=0.6, u=u, pick=pick)
    assert got.tolist() == [2, 2, int(greedy[2]), 1, int(greedy[4])]
    tw = ag.act(obs)
    assert torch.equal(tw, torch.tensor(Q.TWISTS, dtype=torch.float32)[greedy])


def test_checkpoint_round_trip_and_parameter_record(tmp_path):
    ag = _agent(obs_dim=361, hidden=(300, 300), seed=2)
    ag.epsilon = 0.049911691230058335
    ag.memory_size = 1_000_000                                     # (the record's value; the test's ring is small)
    ag.save(str(tmp_path), 1500)
    assert sorted(os.listdir(tmp_path)) == ["dqn_model_ep1500.json", "dqn_model_ep1500.pt"]
    rec = json.load(open(tmp_path / "dqn_model_ep1500.json"))
    ref = {"current_epoch": 1500, "nsteps": 250, "network_inputs": 361, "network_outputs": 3, "memorySize": 1000000,
           "nepisodes": 1500, "network_structure": [300, 300], "discountFactor": 0.99, "learningRate": 0.00025, "learnStart": 64,
           "explorationRate": 0.049911691230058335, "updateTargetNetwork": 10000, "minibatch_size": 64}   # dqn_model_ep1500.json
    assert rec == ref
    sd = torch.load(tmp_path / "dqn_model_ep1500.pt")
    assert list(sd) == ["linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "linear3.weight", "linear3.bias"]
    other = _agent(obs_dim=361, hidden=(300, 300), seed=9)
    other.load_models(str(tmp_path / "dqn_model_ep1500.pt"), str(tmp_path / "dqn_model_ep1500.json"))
    for x, y, z in zip(ag.q.parameters(), other.q.parameters(), other.q_t.parameters()):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert other.epsilon == 0.049911691230058335


def test_epsilon_draw_helper_is_uniform():
    u = np.array([Q.epsilon_draw(5, 3, i) for i in range(6000)])
    assert abs(u[:, 0].mean() - 0.5) < 0.02 and set(u[:, 1].astype(int)) == {0, 1, 2}
    assert np.abs(np.bincount(u[:, 1].astype(int)) / 6000 - 1 / 3).max() < 0.03


@pytest.mark.parametrize("name,cls,nfields", [("cn_dqn_config", "CnDqnConfig", 19), ("cn_dqn_act_io", "CnDqnActIO", 16),
                                               ("cn_dqn_batch", "CnDqnBatch", 6)])
def test_ctypes_layout_matches_the_header(tmp_path, name, cls, nfields):
    from crowdnav import _abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    k = getattr(_abi, cls)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "crowdnav.h"', 'int main(void) {',
             'printf("sizeof %%zu\\n", sizeof(%s));' % name]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], name, f[0]) for f in k._fields_]
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(k)
    for f in k._fields_:
        assert int(got[f[0]]) == getattr(k, f[0]).offset, f[0]
    assert len(k._fields_) == nfields


def test_dqn_entry_points_are_exported():
    import crowdnav
    crowdnav.build()
    L = C.CDLL(crowdnav._abi.LIB_PATH)
    for s in ("cn_dqn_create", "cn_dqn_destroy", "cn_dqn_update", "cn_dqn_loss_dev", "cn_dqn_batch_dev", "cn_dqn_act"):
        assert hasattr(L, s) and s in crowdnav._abi.EXPORTS


def test_trainer_dqn_flags_and_defaults():
    """--algo dqn: obs_layout 1 and nsteps 250 (dqn.yaml) unless given; the DQN flags parse; the other algorithms keep theirs."""
    from crowdnav import train
    a = train.parse_args(["--algo", "dqn", "--dqn-inputs", "363", "--epsilon", "0", "--epsilon-discount", "0.99", "--target-update", "500"])
    assert (a.algo, a.dqn_inputs, a.epsilon, a.epsilon_discount, a.target_update) == ("dqn", 363, 0.0, 0.99, 500)
    assert a.max_steps == 250 and a.obs_layout == 1 and a.out == "runs/dqn"
    d = train.parse_args(["--algo", "dqn"])
    assert (d.dqn_inputs, d.epsilon, d.epsilon_discount, d.target_update) == (361, 1.0, 0.995, 10000)
    assert train.parse_args(["--algo", "dqn", "--max-steps", "90", "--obs-layout", "0"]).max_steps == 90
    t = train.parse_args([])
    assert t.max_steps == 1000 and t.obs_layout is None and t.algo == "td3"
    for bad in (["--algo", "dqn", "--dqn-inputs", "362"], ["--algo", "dqn", "--reset-mode", "same"]):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


G = np.load(os.path.join(os.path.dirname(__file__), "golden", "dqn.npz"))


def _golden_params(prefix):
    return {k: G["%s_%s" % (prefix, k)] for k in ("w1", "b1", "w2", "b2", "w3", "b3")}


@pytest.mark.parametrize("case", ["online", "target"])
def test_golden_batches_from_the_reference(case):
    """deepq.learnOnMiniBatch's own X_batch / Y_batch (tools/make_dqn_goldens.py): the float64 statement and the PyTorch agent
    reproduce them, rows in the same order (final samples' extra rows included), Q' from the net the case names."""
    idx = G[case + "_idx"]
    batch = (G["S"][idx], G["act"][idx], G["rew"][idx], G["S2"][idx], G["fin"][idx] != 0)
    p, pt = _golden_params("p"), _golden_params("pt")
    ut = case == "target"
    X, Y, src = Q.x_batch(*batch, Q.forward(p, batch[0])[0], Q.forward(pt if ut else p, batch[3])[0], 0.99)
    np.testing.assert_array_equal(X, G[case + "_X"])
    np.testing.assert_allclose(Y, G[case + "_Y"], rtol=1e-12, atol=1e-12)
    assert int(G[case + "_bs"]) == len(idx)
    D, H, A, B = [int(x) for x in G["w"]]
    ag = _agent(obs_dim=D, hidden=(H, H), batch_size=B)
    with torch.no_grad():
        for net, pp in ((ag.q, p), (ag.q_t, pt)):
            for k, v in pp.items():
                getattr(getattr(net, "linear%s" % k[1]), "weight" if k[0] == "w" else "bias").copy_(torch.from_numpy(v))
    tb = tuple(torch.from_numpy(np.asarray(x, dtype=np.float32)) for x in batch)
    Xt, Yt, _ = ag.targets(*tb, use_target=ut)
    np.testing.assert_allclose(Xt.double().numpy(), G[case + "_X"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(Yt.double().numpy(), G[case + "_Y"], rtol=1e-5, atol=1e-4)
    other = Q.x_batch(*batch, Q.forward(p, batch[0])[0], Q.forward(p if ut else pt, batch[3])[0], 0.99)[1]
    assert np.abs(other - G[case + "_Y"]).max() > 1e-3                    # the other network's Q' is visibly different


def test_golden_select_action():
    """selectAction (deepq.py:178-184) on the pinned draws: explore where u < epsilon, else np.argmax."""
    ag = _agent(obs_dim=int(G["w"][0]), hidden=(int(G["w"][1]),) * 2)
    with torch.no_grad():
        for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
            getattr(getattr(ag.q, "linear%s" % k[1]), "weight" if k[0] == "w" else "bias").copy_(torch.from_numpy(G["p_" + k]))
    got = ag.select(torch.from_numpy(G["S"][:6]).float(), epsilon=float(G["sel_eps"]), u=torch.from_numpy(G["sel_u"]),
                    pick=torch.from_numpy(G["sel_pick"]))
    assert got.tolist() == G["sel_action"].tolist()
