"""cn_ddpg_update (csrc/crowdnav_ddpg.hip) on the device: the reference's learn() goldens (tests/golden/ddpg.npz), a float64
statement of the same update with the gradients observed (tests/ddpg_f64.py), determinism, the replay path, argument checks,
Adam across four updates against a float64 series (adam_series.run), a hipGraph capture, the DDPG agent in the fused collection loop, and the trainer end to end.

Adam with beta1 = beta2 = 0 steps w' = w - lr g / (|g| + eps); the tests invert that per element.  Both DDPG gradients are taken
at the pre-update weights (ddpg.py:216-239), so ONE call with large learning rates for both optimizers yields the critic's and
the actor's gradients together.  `-s` prints the worst error / bound of every tensor."""
import csv
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest
import torch

import adam_series as A
import ddpg_f64 as D
import td3_f64 as R
from conftest import ROOT
from learner_handle import LearnerHandle, batch_struct, lib, mlp_struct, ring_fields

pytestmark = pytest.mark.gpu

CFG = dict(gamma=0.99, tau=2.0 ** -4, max_v=0.22, max_w=2.0, noise_std=0.25, noise_clip=0.5)
LR = 1024.0
SHAPES = [
    (398, 256, 64), (363, 256, 64),                    # the product: obs_layout 0 and the shipped checkpoints' obs_layout 1
    (46, 32, 16),                                      # the reference's learn() goldens
] + [(45, h, 40) for h in (1, 4, 15, 16, 17, 31, 32, 33, 257)] + [   # hidden around the 16 / 32 tiles, qnt and dant
    (dc - 2, 40, 24) for dc in (3, 15, 16, 17, 31, 32, 33)] + [      # Dc around one and two blocks of 16
    (20, 48, b) for b in (1, 3, 33, 127, 129)] + [                  # batch around the 32-row weight-gradient tile and its 4-row steps
    (398, 256, 4096),                                  # the batch limit
    (398, 4096, 64),                                   # the hidden limit
]
ALL_DONE = (45, 17, 40)                                # y = r in every row
DISCRIMINATE = ((398, 256, 64), (45, 33, 40))
SCALE_ERR = 1e-3


def make_case(shape, seed=0, margins=True):
    obs_dim, hidden, B = shape
    g = torch.Generator().manual_seed(seed + 1000 * hidden + B + 7)
    P = D.new_params(obs_dim, hidden, g, device="cuda")
    s = torch.randn((B, obs_dim), generator=g) * 0.5
    a = torch.stack([torch.rand(B, generator=g) * 0.22, torch.rand(B, generator=g) * 4 - 2], 1)
    r = 2 + 0.5 * torch.randn(B, generator=g)
    s2 = torch.randn((B, obs_dim), generator=g) * 0.5
    d = (torch.rand(B, generator=g) < 0.3).float()
    if shape == ALL_DONE:
        d[:] = 1
    elif B >= 2:
        d[0], d[1] = 0, 1
    batch = tuple(x.float().cuda().contiguous() for x in (s, a, r, s2, d))
    nz = torch.randn((B, 2), generator=g).double().cuda()          # only for the "target noise" wrong variant
    dead = D.plant_dead_units(P, hidden) if margins else {}
    N = R.chain_length(*shape)
    if margins:
        D.establish_margins(P, batch, CFG, N)
    return P, batch, nz, N, dead


class Fused(LearnerHandle):
    """One cn_ddpg handle on its own float32 copies of the parameters."""

    def __init__(self, P, shape, lr_c, lr_a, eps, beta1=0.0, beta2=0.0, tau=CFG["tau"], replay=None):
        self.P = {n: {k: v.detach().clone().contiguous() for k, v in p.items()} for n, p in P.items()}
        cfg = lib()[0].CnDdpgConfig(obs_dim=shape[0], hidden=shape[1], batch=shape[2], gamma=CFG["gamma"], tau=tau, lr_actor=lr_a,
                                    lr_critic=lr_c, beta1=beta1, beta2=beta2, eps=eps, max_v=CFG["max_v"], max_w=CFG["max_w"], seed=7,
                                    **{n: mlp_struct(self.P[n], R.NAMES) for n in D.NETS}, **ring_fields(replay))
        super().__init__("ddpg", cfg, (self.P, replay))

    def update(self, batch, sync=True):
        super().update(batch=batch_struct(batch), sync=sync)

    def loss(self):
        return float(super().loss())


def test_fused_ddpg_update_on_the_reference_learn_goldens():
    """The golden vectors of the REFERENCE's own ddpg.Agent.learn() (tests/golden/ddpg.npz, tools/make_ddpg_goldens.py) through
    cn_ddpg_update: four updates on the pinned batch, at the tolerances of the fused TD3 update's golden test."""
    from crowdnav.ddpg import Agent
    G = np.load(os.path.join(ROOT, "tests", "golden", "ddpg.npz"))
    ag = Agent(device="cuda", memory_size=64, obs_dim=46, hidden=32, batch_size=16)
    nets = dict(actor=ag.actor, actor_t=ag.actor_t, critic=ag.critic, critic_t=ag.critic_t)
    for k, m in nets.items():
        m.load_state_dict({n: torch.from_numpy(G["init.%s.%s" % (k, n)]).cuda() for n in m.state_dict()})
    ag.enable_fused_update()
    dev = lambda x: torch.from_numpy(x).cuda()
    batch = (dev(G["upd_s"]), dev(G["upd_a"]), dev(G["upd_r"])[:, None], dev(G["upd_s2"]), dev(G["upd_d"])[:, None])
    losses = []
    for step in range(4):
        losses.append(ag.learn(step, batch=batch))
        torch.cuda.synchronize()
        for k, m_ in nets.items():
            for n, v in m_.state_dict().items():
                np.testing.assert_allclose(v.cpu().numpy(), G["step%d.%s.%s" % (step, k, n)], rtol=5e-4, atol=2e-6, err_msg="step %d %s.%s" % (step, k, n))
    vals = [float(l) for l in losses]
    np.testing.assert_allclose(vals, G["loss"], rtol=1e-5, atol=0)
    assert len({l.data_ptr() for l in losses}) == 4
    del ag
    assert [float(l) for l in losses] == vals


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_fused_ddpg_gradients_loss_and_soft_updates_match_float64(shape):
    report = []
    try:
        _gradients(shape, report)
    finally:
        print("\n".join(report))


def _gradients(shape, report):
    obs_dim, hidden, B = shape
    P0, batch, nz, N, dead = make_case(shape)
    assert D.margin_report(P0, batch, CFG, N) >= 1.0
    P64, b64 = R.to64(P0), R.batch_double(batch)
    refc = D.critic_grads(P64, b64, CFG)
    refa = D.actor_grads(P64, b64[0], CFG, N_mask=N)
    assert refa["flip_rows"] == 0
    t = refc["t"]
    if shape == ALL_DONE:
        assert torch.equal(t["y"], b64[2])
    elif B >= 2:
        assert 0 < float(b64[4].mean()) < 1
    assert float(R.actor_fwd(P64["actor"], b64[0], CFG)["logits"].abs().max()) >= 7.0
    eps_c = A.pow2_at_least(max(float(v.abs().max()) for v in refc["g"].values()))
    eps_a = A.pow2_at_least(max(float(v.abs().max()) for v in refa["g"].values()))
    lr_c, lr_a = LR, LR * eps_c / eps_a          # the actor's step as large relative to its gradient as the critic's (powers of two)
    k_ = Fused(P0, shape, lr_c, lr_a, eps_c)
    k_.update(batch)
    P1, loss = k_.P, k_.loss()
    k_.close()
    l_ = float(refc["loss"])
    report.append("%s: loss %.9g float64 %.9g" % (shape, loss, l_))
    assert abs(loss - l_) <= 1e-5 * abs(l_), (loss, l_)
    for net, ref, lr in (("critic", refc, lr_c), ("actor", refa, lr_a)):
        g, extra = R.recover(P0, P1, net, lr, eps_c)
        ratios = R.compare_grads(g, ref["g"], ref["bound"], extra)
        report.append("%-7s worst/bound " % net + " ".join("%s %.3g" % kv for kv in ratios.items()))
        assert R.accept(ratios), (net, ratios)
        R.check_dead(P0, P1, net, dead)
        R.rejects_gross(g, ref, extra, net)
        if net == "critic":
            gc, xc = g, extra
        else:
            ga, xa = g, extra
    if hidden >= 4:
        assert any(bool((v != 0).any()) for v in refa["g"].values())
    # soft updates from the STEPPED weights (ddpg.py:241-254)
    for tg, src in (("critic_t", "critic"), ("actor_t", "actor")):
        for k in R.NAMES:
            t0 = P0[tg][k].double()
            want = R.soft_update(t0, P1[src][k].double(), CFG["tau"])
            assert R.worst_ratio(P1[tg][k], want, R.soft_bound(t0, P1[src][k].double(), CFG["tau"])) <= 1.0, (tg, k)
    if shape in DISCRIMINATE:
        # the actor's gradient fits the pre-update critic and NOT the critic this very update produced (TD3's order)
        post = D.actor_grads(P64, b64[0], CFG, critic=R.to64(P1)["critic"])
        assert not R.accept(R.compare_grads(ga, post["g"], post["bound"], xa)), "actor through the post-update critic accepted"
        for wrong in ("twin", "noise"):
            w = D.critic_grads(P64, b64, CFG, y_from=wrong, nz=nz)
            assert not R.accept(R.compare_grads(gc, w["g"], w["bound"], xc)), "y = %s accepted" % wrong
        for net, ref, g, x in (("critic", refc, gc, xc), ("actor", refa, ga, xa)):
            scaled = {kk: v * (1 + SCALE_ERR) for kk, v in ref["g"].items()}
            assert not R.accept(R.compare_grads(g, scaled, ref["bound"], x)), "%s x (1 + %g) accepted" % (net, SCALE_ERR)


class _SeriesHandle(Fused):
    """adam_series.run's learner: one cn_ddpg handle; read() / write() copy from / into the device tensors it points at."""

    def __init__(self, P, shape, hp):
        super().__init__(P, shape, hp["lr_critic"], hp["lr_actor"], hp["eps"], beta1=hp["beta1"], beta2=hp["beta2"], tau=hp["tau"])

    def read(self):
        return {n: {k: v.clone() for k, v in p.items()} for n, p in self.P.items()}

    def write(self, P):
        for n in P:
            for k in P[n]:
                self.P[n][k].copy_(P[n][k])


@pytest.mark.parametrize("case", D.SERIES_CASES, ids=D.series_id)
def test_fused_ddpg_adam_across_four_updates_matches_float64(case):
    """Four updates (both optimisers step on every one: adam_args(.., 1)) beside ddpg_f64's float64 series: every tensor of the
    four networks within its bound after every update, each wrong variant (a bias correction frozen at t = 1, moments not
    carried, betas exchanged, one lr for both, targets from the pre-step weights) rejected on each network it concerns, dead
    units bit for bit, and a new handle on the stepped parameters stepping as a fresh Adam.  Betas 0.5 / 0.75 and the product's;
    eps a power of two >= twice the first update's largest gradient element, re-asserted before every update; two different
    power-of-two learning rates; tau = 2^-4.  Moments are observed only through the weights, and the margins are re-established
    between updates: not a free-running trajectory.  tests/test_ddpg_f64_helpers.py runs the same cases on the CPU."""
    shape, betas = case
    res = A.run(D.series(shape, betas, device="cuda", cfg=dict(CFG)), _SeriesHandle)
    print("worst/bound %s; smallest rejecting ratio %s" % ({n: "%.3g" % v for n, v in res["worst"].items()}, {k: "%.3g" % v for k, v in res["rejected"].items()}))
    assert max(res["worst"].values()) <= 1.0


def test_cn_ddpg_create_and_update_reject_bad_arguments():
    _abi, L = lib()
    z = torch.zeros(16, device="cuda")
    m = _abi.CnTd3Mlp(*([z.data_ptr()] * 6))
    for obs_dim, hidden, batch in ((8, 16, 0), (8, 16, 4097), (8, 0, 16), (8, 4097, 16), (0, 16, 16)):
        cfg = _abi.CnDdpgConfig(obs_dim=obs_dim, hidden=hidden, batch=batch, actor=m, actor_t=m, critic=m, critic_t=m)
        h = C.c_void_p()
        assert L.cn_ddpg_create(C.byref(cfg), 0, C.byref(h)) == -2            # CN_ERR_CONFIG
        assert b"out of range" in L.cn_td3_last_error()
        assert not h.value
    shape = (20, 16, 8)
    P0, batch, _, _, _ = make_case(shape, margins=False)
    k_ = Fused(P0, shape, 1e-3, 1e-4, 1e-8)
    try:
        noise = torch.zeros((8, 2), device="cuda")
        bp = _abi.CnTd3Batch(*[x.data_ptr() for x in batch], noise.data_ptr())
        assert L.cn_ddpg_update(k_.h, C.byref(bp), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0
        assert b"target_noise" in L.cn_td3_last_error()
        assert L.cn_ddpg_update(k_.h, None, None) != 0                  # no batch and no replay ring
        torch.cuda.synchronize()
        assert all(R.same(P0, k_.P, n) for n in D.NETS)                  # nothing was enqueued
    finally:
        k_.close()


def test_two_handles_on_identical_parameters_end_bit_identical():
    shape = (45, 33, 40)
    P0, batch, _, _, _ = make_case(shape, margins=False)
    a = Fused(P0, shape, 1e-3, 1e-4, 1e-8, beta1=0.9, beta2=0.999, tau=0.001)
    b = Fused(P0, shape, 1e-3, 1e-4, 1e-8, beta1=0.9, beta2=0.999, tau=0.001)
    try:
        for _ in range(4):
            a.update(batch)
            b.update(batch)
        assert all(R.same(a.P, b.P, n) for n in D.NETS)
        assert a.loss() == b.loss()
        assert not R.same(P0, a.P, "critic") and not R.same(P0, a.P, "actor_t")
    finally:
        a.close(); b.close()


def _ring(shape, cap, size, fill=float("nan"), seed=3):
    obs_dim, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    ring = dict(s=torch.randn((cap, obs_dim), generator=g) * 0.5, a=torch.rand((cap, 2), generator=g),
                r=torch.randn(cap, generator=g), s2=torch.randn((cap, obs_dim), generator=g) * 0.5, d=(torch.rand(cap, generator=g) < 0.3).float())
    if fill is not None:
        for k in ring:
            ring[k][size:] = fill
    ring = {k: v.float().cuda().contiguous() for k, v in ring.items()}
    ring["size"] = torch.tensor([size], dtype=torch.int64, device="cuda")
    return ring


def test_replay_path_samples_only_live_rows():
    """batch == NULL: (a) a ring of live size 1 equals an explicit batch of B copies of row 0, bit for bit; (b) *size_dev = 0
    equals size 1; (c) rows [size, capacity) full of NaN or of 1e30 never reach the weights or the loss."""
    shape = (45, 33, 40)
    B = shape[2]
    P0, _, _, _, _ = make_case(shape, margins=False)
    args = dict(lr_c=1e-3, lr_a=1e-4, eps=1e-8, beta1=0.9, beta2=0.999, tau=0.001)
    ring1, ring0, ringx = _ring(shape, 64, 1), _ring(shape, 64, 1), _ring(shape, 64, 1)
    ring0["size"].zero_()
    batch = tuple(ringx[k][:1].expand((B,) + ringx[k].shape[1:]).contiguous() for k in ("s", "a", "r", "s2", "d"))
    hs = [Fused(P0, shape, replay=ring1, **args), Fused(P0, shape, replay=ring0, **args), Fused(P0, shape, **args)]
    try:
        for _ in range(3):
            hs[0].update(None); hs[1].update(None); hs[2].update(batch)
        assert all(R.same(hs[0].P, hs[2].P, n) for n in D.NETS)
        assert all(R.same(hs[0].P, hs[1].P, n) for n in D.NETS)
    finally:
        for h in hs:
            h.close()
    for fill in (float("nan"), 1e30):
        for size in (1, 37, 63, 64):
            h = Fused(P0, shape, replay=_ring(shape, 64, size, fill=fill), **args)
            try:
                for step in range(4):
                    h.update(None)
                    assert h.loss() < 1e3, (fill, size, step, h.loss())
                assert all(bool(torch.isfinite(v).all()) for p in h.P.values() for v in p.values()), (fill, size)
                assert not R.same(P0, h.P, "critic")
            finally:
                h.close()


def test_graph_capture_of_the_update_replays_bit_for_bit():
    """cn_ddpg_update enqueues only and reads nothing from the host: one update captured into a hipGraph (one stream, a straight
    chain of launches) and replayed three times equals three eager updates, weights and loss bit for bit."""
    shape = (398, 256, 64)
    P0, _, _, _, _ = make_case(shape, margins=False)
    args = dict(lr_c=1e-3, lr_a=1e-4, eps=1e-8, beta1=0.9, beta2=0.999, tau=0.001)
    ring = _ring(shape, 512, 300, fill=None)
    eager, graphed = Fused(P0, shape, replay=ring, **args), Fused(P0, shape, replay=ring, **args)
    try:
        for _ in range(3):
            eager.update(None)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.update(None, sync=False)
        torch.cuda.synchronize()
        assert all(R.same(P0, graphed.P, n) for n in D.NETS)         # capturing ran nothing
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert all(R.same(eager.P, graphed.P, n) for n in D.NETS)
        assert eager.loss() == graphed.loss()
    finally:
        eager.close(); graphed.close()


@pytest.mark.parametrize("obs_layout", [0, 1])
def test_ddpg_agent_in_collect_policy_equals_act_then_step(obs_layout):
    """crowdnav.rollout.collect_policy with a DDPG agent (explore_sigma 0: the reference's add_noise=False) leaves the replay ring
    and the env exactly where the per-step loop act_mfma -> step -> add_masked leaves them, on both observation layouts."""
    from crowdnav import Config
    from crowdnav.ddpg import Agent
    from crowdnav.env import VecEnv
    from crowdnav.rollout import collect_policy
    N, steps = 96, 53
    cfg = Config(n_envs=N, max_steps=12, seed=21, ped_cycle_ms=1400, obs_layout=obs_layout)
    e1, e2 = VecEnv(cfg), VecEnv(cfg)
    a1 = Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=3, memory_size=4000)
    a2 = Agent(obs_dim=cfg.obs_dim, device="cuda:0", seed=3, memory_size=4000)
    assert a1.explore_sigma == 0.0
    assert collect_policy(e1, a1, steps, periods=8) == steps * N
    a2.sync_fused_weights()
    obs = e2.reset()
    act = torch.zeros((N, 2), device="cuda")
    resetting = torch.zeros(N, dtype=torch.bool, device="cuda")
    for t in range(steps):
        a2.act_mfma(obs, out=act)
        if t == 0:     # sigma 0: the fused actor is the deterministic policy
            torch.testing.assert_close(act, a2.act(obs), rtol=0, atol=1e-5)
        prev = obs.clone()
        obs, reward, done = e2.step(act, auto_reset="next")
        a2.memory.add_masked(prev, act, reward, obs, done, ~resetting)
        resetting = done.bool()
    torch.cuda.synchronize()
    m1, m2 = a1.memory, a2.memory
    assert m1.sync_len() == m2.sync_len() and 0 < len(m2) < steps * N and m1.pos == m2.pos
    n = len(m2)
    for x, y in ((m1.s, m2.s), (m1.a, m2.a), (m1.r, m2.r), (m1.s2, m2.s2), (m1.d, m2.d)):
        assert torch.equal(x[:n], y[:n])
    assert torch.equal(e1.obs, e2.obs) and torch.equal(e1.done, e2.done) and np.array_equal(e1.snapshot(), e2.snapshot())


@pytest.mark.parametrize("variant", ["fused", "torch_ou_layout1"])
def test_trainer_runs_ddpg_end_to_end_and_evaluates_its_checkpoint(tmp_path, variant):
    """python -m crowdnav.train --algo ddpg: a few hundred launches of 64 envs, DDPG checkpoints (target networks,
    ddpg_{actor,critic}_model_ep<N>.pt) and latest_checkpoint.txt, the 8-column ddpg_training.csv, finite losses; --evaluate
    reloads the checkpoint.  The second variant: the PyTorch learner, OU noise (the act -> step loop) and obs_layout 1 (363
    inputs, the shipped checkpoints' layout) for training and evaluation."""
    from crowdnav import train as T
    out = str(tmp_path / "run")
    argv = ["--algo", "ddpg", "--scenario", "bench", "--envs", "64", "--launches", "200", "--max-steps", "25", "--updates", "1",
            "--memory", "20000", "--log-every", "50", "--checkpoint-every", "100", "--seed", "3", "--csv", "--out", out]
    if variant == "fused":
        argv += ["--learner", "fused"]
    else:
        argv += ["--learner", "torch", "--ou-noise", "--obs-layout", "1"]
    agent, episodes = T.main(argv)
    from crowdnav.ddpg import Agent
    assert isinstance(agent, Agent) and agent.batch_size == 64 and agent.tau == 0.001
    assert agent.actor.linear1.in_features == (363 if variant != "fused" else 398)
    assert episodes > 64
    if variant == "fused":
        assert getattr(agent, "_fused", None) and agent._fused.h
    else:
        assert float(agent.noise.state.abs().max()) > 0          # OU states moved (and were reset per finished episode)
    latest = int(open(os.path.join(out, "latest_checkpoint.txt")).read().split()[0])
    assert latest == episodes
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "ddpg_*_model_ep*.pt")))
    assert "ddpg_actor_model_ep%d.pt" % latest in names and "ddpg_critic_model_ep%d.pt" % latest in names
    assert not glob.glob(os.path.join(out, "td3_*"))
    rows = list(csv.reader(open(os.path.join(out, "ddpg_training.csv"))))
    assert rows[0] == ["episode_number", "success_episode", "failure_episode", "episode_reward", "episode_step", "ego_safety_score",
                       "social_safety_score", "timelapse"] and len(rows) - 1 == episodes
    assert all(len(r) == 8 for r in rows)
    sd = torch.load(os.path.join(out, "ddpg_actor_model_ep%d.pt" % latest), map_location="cuda")
    for k, v in agent.actor_t.state_dict().items():
        assert torch.equal(sd[k], v)                             # the target network was saved (DDPG:262-266)
    loss = agent.learn()                                          # (after the comparison: an update moves the targets)
    assert loss is not None and math.isfinite(float(loss))
    assert all(bool(torch.isfinite(p).all()) for m in (agent.actor, agent.critic, agent.actor_t, agent.critic_t) for p in m.parameters())
    ev = ["--algo", "ddpg", "--evaluate", "--load", out, "--scenario", "bench", "--envs", "32", "--max-steps", "20", "--seed", "4",
          "--out", out]
    if variant != "fused":
        ev += ["--obs-layout", "1"]
    st = T.main(ev)
    assert len(st.rows) == 32
    assert os.path.exists(os.path.join(out, "ddpg_training_test_bench.csv"))
