"""cn_dqn_act and cn_dqn_update (csrc/crowdnav_dqn.hip) on the device against a float64 statement of the reference's DQN
(tests/dqn_f64.py): Q values, argmax and the epsilon draw; the update's gradients read back from an invertible RMSprop step, its
two chunks, the target-net switch and copy; determinism, a hipGraph capture and the replay path.

RMSprop with rho = 0 steps w' = w - lr g / (|g| + eps); with lr = eps = 1 the tests invert that per element: g = d / (1 - |d|)."""
import numpy as np
import pytest
import torch

import dqn_f64 as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _agent(D=361, ld=363, H=300, B=64, **kw):
    from crowdnav.dqn import Agent
    kw.setdefault("memory_size", 256)
    return Agent(obs_dim=D, obs_ld=ld, hidden=(H, H), batch_size=B, device=DEV, **kw)


def _params(net):
    return {k: getattr(getattr(net, "linear%d" % int(k[1])), "weight" if k[0] == "w" else "bias").detach().double().cpu().numpy()
            for k in ("w1", "b1", "w2", "b2", "w3", "b3")}


def _batch(B, ld, n_final, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand((B, ld), generator=g) * 3.5
    s2 = torch.rand((B, ld), generator=g) * 3.5
    a = torch.randint(0, 3, (B,), generator=g)
    r = torch.randn(B, generator=g) * 10
    d = torch.zeros(B)
    d[torch.randperm(B, generator=g)[:n_final]] = 1.0
    return s, a, r, s2, d


def _np(batch, D):
    s, a, r, s2, d = batch
    return (s[:, :D].double().numpy(), a.numpy(), r.double().numpy(), s2[:, :D].double().numpy(), d.numpy() != 0)


def _recover(p0, p1):
    dlt = p0 - p1
    return dlt / (1.0 - np.abs(dlt))


def _close(got, want, rel):
    scale = max(np.abs(want).max(), 1e-30)
    return np.abs(got - want).max() / scale <= rel


# ---- cn_dqn_act ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,ld", [(1, 361, 363), (16, 361, 363), (4096, 361, 363), (37, 363, 363), (5, 17, 20)])
def test_act_q_and_argmax_against_f64(n, D, ld):
    ag = _agent(D=D, ld=ld, H=300 if D > 20 else 33, seed=n)
    obs = torch.rand((n, ld), generator=torch.Generator().manual_seed(n)) * 3.5
    q = torch.zeros((n, 3), device=DEV)
    idx, tw = ag.act_fused(obs.to(DEV), epsilon=0.0, q_out=q)
    torch.cuda.synchronize()
    p = _params(ag.q)
    want = Q.forward(p, obs[:, :D].double().numpy())[0]
    got = q.cpu().double().numpy()
    err = np.abs(got - want)
    bound = 1e-4 * (1.0 + np.abs(want).max())
    assert err.max() <= bound, (err.max(), bound)
    srt = np.sort(want, 1)
    clear = (srt[:, 2] - srt[:, 1]) > 4 * bound
    assert clear.mean() > 0.5
    assert np.array_equal(idx.cpu().numpy()[clear], np.argmax(want, 1)[clear])
    assert np.array_equal(tw.cpu().numpy(), Q.TWISTS[idx.cpu().numpy()].astype(np.float32))


def test_act_ties_go_to_the_lowest_index():
    ag = _agent(D=8, ld=8, H=32)
    with torch.no_grad():
        ag.q.linear3.weight.zero_(); ag.q.linear3.bias.copy_(torch.tensor([1.0, 1.0, 1.0]))
    idx, _ = ag.act_fused(torch.rand((40, 8), device=DEV), epsilon=0.0)
    assert (idx == 0).all()
    with torch.no_grad():
        ag.q.linear3.bias.copy_(torch.tensor([0.0, 2.0, 2.0]))
    idx, _ = ag.act_fused(torch.rand((40, 8), device=DEV), epsilon=0.0)
    assert (idx == 1).all()


def test_act_epsilon_one_is_uniform_and_draws_are_deterministic():
    ag = _agent(D=361, ld=363, H=300)
    n = 30000
    obs = torch.rand((n, 363), device=DEV)
    ag._act_calls = 7
    idx, tw = ag.act_fused(obs, epsilon=1.0)
    ag._act_calls = 7
    idx2, _ = ag.act_fused(obs, epsilon=1.0)
    cnt = torch.bincount(idx.long(), minlength=3).cpu().numpy()
    chi2 = ((cnt - n / 3) ** 2 / (n / 3)).sum()
    assert chi2 < 13.8, cnt                                       # p = 0.001 at 2 degrees of freedom
    assert torch.equal(idx, idx2)
    want = np.array([Q.epsilon_draw(ag._act_seed, 7, i)[1] for i in range(200)])
    assert np.array_equal(idx[:200].cpu().numpy(), want)
    assert np.array_equal(tw.cpu().numpy(), Q.TWISTS[idx.cpu().numpy()].astype(np.float32))


def test_act_epsilon_schedule_on_the_device():
    """episodes_dev: epsilon0 * 0.995^(E + 1) while > 0.05 -- rows explore exactly where the keyed uniform is below it."""
    from crowdnav.dqn import epsilon_after
    ag = _agent(D=16, ld=16, H=32, epsilon=1.0)
    n = 2000
    obs = torch.rand((n, 16), device=DEV)
    for E in (0, 137, 1499, 5000):
        e = epsilon_after(E + 1)
        ag._act_calls = 3
        idx_g, _ = ag.act_fused(obs, epsilon=0.0)
        ag._act_calls = 3
        idx, _ = ag.act_fused(obs, episodes_dev=torch.tensor(E, dtype=torch.int64, device=DEV))
        u = np.array([Q.epsilon_draw(ag._act_seed, 3, i) for i in range(n)])
        want = np.where(u[:, 0] < e, u[:, 1], idx_g.cpu().numpy())
        assert np.array_equal(idx.cpu().numpy(), want), E


# ---- cn_dqn_update ---------------------------------------------------------------------------------------------------------
def _run_update(ag, batch, perm):
    ag.enable_fused_update()
    ag.learn(batch=tuple(t.to(DEV) for t in batch), perm=perm)
    torch.cuda.synchronize()


@pytest.mark.parametrize("D,ld,H,B", [(361, 363, 300, 64), (33, 35, 47, 17)])
def test_update_gradients_against_f64_no_final(D, ld, H, B):
    """F = 0: one RMSprop step (rho = 0, lr = eps = 1) gives every gradient back; Y uses the online net before the first copy."""
    ag = _agent(D=D, ld=ld, H=H, B=B, lr=1.0, rho=0.0, eps=1.0, seed=3)
    with torch.no_grad():                                         # a target net that differs, to see which one Q' reads
        for t in ag.q_t.parameters():
            t.mul_(1.5)
    batch = _batch(B, ld, 0, seed=B)
    p0 = _params(ag.q)
    pt = _params(ag.q_t)
    perm = np.random.default_rng(0).permutation(B)
    _run_update(ag, batch, perm)
    p1 = _params(ag.q)
    acc0 = {k: np.zeros_like(v) for k, v in p0.items()}
    _, _, info = Q.update(p0, pt, acc0, _np(batch, D), perm, 0.99, 1.0, 0.0, 1.0, use_target=False)
    _, _, wrong = Q.update(p0, pt, acc0, _np(batch, D), perm, 0.99, 1.0, 0.0, 1.0, use_target=False, variant="target_early")
    for k in p0:
        g = _recover(p0[k], p1[k])
        assert _close(g, info["g1"][k], 2e-3), k
    assert not _close(_recover(p0["w3"], p1["w3"]), wrong["g1"]["w3"], 2e-2)
    assert torch.equal(ag.q_t.linear1.weight.cpu(), torch.from_numpy(pt["w1"]).float())


@pytest.mark.parametrize("D,ld,H,B,nf", [(361, 363, 300, 64, 9), (33, 35, 47, 17, 5)])
def test_update_two_chunks_against_f64(D, ld, H, B, nf):
    """F > 0: the second step on the stepped weights, all three columns of chunk 2, against the Y from before either step."""
    ag = _agent(D=D, ld=ld, H=H, B=B, lr=1.0, rho=0.0, eps=1.0, seed=5)
    batch = _batch(B, ld, nf, seed=B + 1)
    p0 = _params(ag.q)
    perm = np.random.default_rng(1).permutation(B + nf)
    _run_update(ag, batch, perm)
    p2 = _params(ag.q)
    acc0 = {k: np.zeros_like(v) for k, v in p0.items()}
    args = (p0, p0, acc0, _np(batch, D), perm, 0.99, 1.0, 0.0, 1.0, False)
    want, _, info = Q.update(*args)
    assert len(info["src"]) == B + nf
    Y = ag.fused_batch(6, (2 * B, 3)).double().numpy()
    Ywant = np.zeros((2 * B, 3)); Ywant[info["src"]] = info["Y"]
    rows = info["src"]
    assert np.abs(Y[rows] - Ywant[rows]).max() <= 1e-4 * (1 + np.abs(Ywant).max())
    q_pre = ag.fused_batch(7, (2 * B, 3)).double().numpy()           # chunk 1's forward, kept after chunk 2's
    q_want = np.concatenate([Q.forward(p0, _np(batch, D)[0])[0], Q.forward(p0, _np(batch, D)[3])[0]])
    assert np.abs(q_pre - q_want).max() <= 1e-4 * (1 + np.abs(q_want).max())
    chunk = ag.fused_batch(4, (2 * B,), torch.int32).numpy()
    assert (chunk[rows[perm[:B]]] == 1).all() and (chunk[rows[perm[B:]]] == 2).all() and (chunk > 0).sum() == B + nf
    for k in p0:
        scale = np.abs(want[k] - p0[k]).max()
        assert np.abs(p2[k] - want[k]).max() <= 2e-3 * scale, k
    for v in ("chosen_only", "skip_chunk2"):
        wrong = Q.update(*args, variant=v)[0]
        bad = max(np.abs(p2[k] - wrong[k]).max() / np.abs(want[k] - p0[k]).max() for k in p0)
        assert bad > 2e-2, v


def test_update_no_phantom_step_and_eps_outside_the_sqrt():
    """Two F = 0 updates with rho = 0.5: a zero-gradient second step would decay the accumulator and change the second update;
    eps inside the square root changes the first."""
    D, ld, H, B = 40, 40, 48, 16
    ag = _agent(D=D, ld=ld, H=H, B=B, lr=1e-2, rho=0.5, eps=1e-3, seed=9)
    p = _params(ag.q)
    acc = {k: np.zeros_like(v) for k, v in p.items()}
    ref = (p, acc)
    wrong = dict(ph=(p, acc), es=(p, acc))
    ag.enable_fused_update()
    for u in range(2):
        batch = _batch(B, ld, 0, seed=100 + u)
        perm = np.arange(B)
        ag.learn(batch=tuple(t.to(DEV) for t in batch), perm=perm)
        nb = _np(batch, D)
        ref = Q.update(ref[0], ref[0], ref[1], nb, perm, 0.99, 1e-2, 0.5, 1e-3, False)[:2]
        for name, v in (("ph", "phantom"), ("es", "eps_in_sqrt")):
            wp, wa = wrong[name]
            wrong[name] = Q.update(wp, wp, wa, nb, perm, 0.99, 1e-2, 0.5, 1e-3, False, variant=v)[:2]
    torch.cuda.synchronize()
    got = _params(ag.q)
    for k in got:
        step = np.abs(ref[0][k] - p[k]).max()
        assert np.abs(got[k] - ref[0][k]).max() <= 1e-3 * step, k
    for name, (wp, _) in wrong.items():
        assert max(np.abs(got[k] - wp[k]).max() / np.abs(ref[0][k] - p[k]).max() for k in got) > 1e-2, name


def test_target_copy_and_switch_at_target_every():
    """target_every = 3: updates 0-2 read Q' from the online net, the copy follows update 2, update 3 reads the target."""
    D, ld, H, B = 24, 24, 32, 8
    ag = _agent(D=D, ld=ld, H=H, B=B, target_update=3, seed=2)
    with torch.no_grad():
        for t in ag.q_t.parameters():
            t.add_(0.25)
    ag.enable_fused_update()
    for u in range(4):
        ag.learn(batch=tuple(t.to(DEV) for t in _batch(B, ld, 2, seed=u)))
        torch.cuda.synchronize()
        fl = ag.fused_batch(5, (8,), torch.int32).numpy()
        assert fl[0] == 1 and fl[3] == (1 if u >= 3 else 0) and fl[4] == (1 if u == 2 else 0), (u, fl)
        if u == 2:
            for a_, b_ in zip(ag.q.parameters(), ag.q_t.parameters()):
                assert torch.equal(a_, b_)
    assert int(ag.fused_batch(8, (1,), torch.int64)[0]) == 4


def _fresh_pair(seed=4, **kw):
    a1 = _agent(D=361, ld=363, H=300, B=64, seed=seed, **kw)
    a2 = _agent(D=361, ld=363, H=300, B=64, seed=seed, **kw)
    return a1, a2


def test_two_handles_bit_identical_and_graph_replay():
    a1, a2 = _fresh_pair()
    batches = [tuple(t.to(DEV) for t in _batch(64, 363, k % 5, seed=20 + k)) for k in range(6)]
    for ag in (a1, a2):
        ag.enable_fused_update()
    for b in batches:
        a1.learn(batch=b); a2.learn(batch=b)
    torch.cuda.synchronize()
    for x, y in zip(a1.q.parameters(), a2.q.parameters()):
        assert torch.equal(x, y)
    # capture a replay-path update into a graph: replays equal eager calls bit for bit
    a3, a4 = _fresh_pair(seed=6, memory_size=4096)
    for ag in (a3, a4):
        g = torch.Generator().manual_seed(1)
        n = 500
        s = torch.rand((n, 363), generator=g).to(DEV); s2 = torch.rand((n, 363), generator=g).to(DEV)
        act = torch.zeros((n, 2), device=DEV); act[:, 0] = torch.randint(0, 3, (n,), generator=g).float().to(DEV)
        ag.memory.add(s, act, torch.randn(n, generator=g).to(DEV), s2, (torch.rand(n, generator=g) < 0.1).to(DEV))
        ag.enable_fused_update()
    torch.cuda.synchronize()
    a3.learn()                                                    # warm-up outside capture on both
    a4.learn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            a3.learn()
    torch.cuda.current_stream().wait_stream(st)
    for _ in range(5):
        graph.replay()
        a4.learn()
    torch.cuda.synchronize()
    for x, y in zip(a3.q.parameters(), a4.q.parameters()):
        assert torch.equal(x, y)
    assert int(a3.fused_batch(8, (1,), torch.int64)[0]) == 6


def test_replay_path_samples_live_rows_and_waits_for_learn_start():
    ag = _agent(D=16, ld=20, H=32, B=8, learn_start=10, memory_size=64, seed=1)
    ag.enable_fused_update()
    n = 10
    s = torch.rand((n, 20), device=DEV) + 1.0
    act = torch.zeros((n, 2), device=DEV); act[:, 0] = torch.arange(n, device=DEV).remainder(3).float()
    ag.memory.add(s, act, torch.arange(n, device=DEV).float(), s + 1, torch.zeros(n, device=DEV))
    w0 = ag.q.linear1.weight.clone()
    ag._fused_learn()                                             # 10 rows: not more than learn_start -> nothing moves
    torch.cuda.synchronize()
    assert torch.equal(w0, ag.q.linear1.weight) and int(ag.fused_batch(8, (1,), torch.int64)[0]) == 0
    ag.memory.add(s[:1] * 0 + 5, act[:1] * 0, torch.tensor([10.0], device=DEV), s[:1], torch.ones(1, device=DEV))
    for _ in range(20):
        ag._fused_learn()
        torch.cuda.synchronize()
        r = ag.fused_batch(1, (8,)).numpy()
        a = ag.fused_batch(3, (8,), torch.int32).numpy()
        x = ag.fused_batch(0, (16, 20)).numpy()[:, :16]             # the gathered [s; s2] rows: live rows hold values >= 1
        assert (x >= 1.0).all(), "a row past the fill level was sampled"
        assert set(r.astype(int).tolist()) <= set(range(11))
        assert np.array_equal(a, np.where(r.astype(int) == 10, 0, r.astype(int) % 3))
    assert not torch.equal(w0, ag.q.linear1.weight)


def test_trainer_end_to_end(tmp_path):
    from crowdnav import train
    out = str(tmp_path / "dqn")
    agent, episodes = train.main(["--algo", "dqn", "--envs", "16", "--launches", "300", "--updates", "4", "--log-every", "100",
                                  "--scenario", "training_as_logged", "--waypoint-reward", "0", "--csv", "--out", out,
                                  "--learner", "fused", "--epsilon", "1.0"])
    assert episodes > 0
    import os
    assert os.path.exists(os.path.join(out, "dqn_training.csv"))
    st = train.main(["--algo", "dqn", "--evaluate", "--load", out, "--envs", "4", "--scenario", "crossing_4", "--max-steps", "60"])
    assert len(st.rows) == 4


def test_golden_batch_through_the_device():
    """The reference's own X_batch / Y_batch (tests/golden/dqn.npz, online case): the device's Y in the same rows."""
    import os
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "dqn.npz"))
    D, H, A, B = [int(x) for x in G["w"]]
    ag = _agent(D=D, ld=D, H=H, B=B)
    with torch.no_grad():
        for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
            for net, pre in ((ag.q, "p_"), (ag.q_t, "pt_")):
                getattr(getattr(net, "linear%s" % k[1]), "weight" if k[0] == "w" else "bias").copy_(torch.from_numpy(G[pre + k]))
    idx = G["online_idx"]
    f32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    batch = (f32(G["S"][idx]), torch.from_numpy(G["act"][idx].astype(np.int64)), f32(G["rew"][idx]), f32(G["S2"][idx]), f32(G["fin"][idx]))
    _run_update(ag, batch, np.arange(len(G["online_X"])))
    src = Q.x_batch(G["S"][idx], G["act"][idx], G["rew"][idx], G["S2"][idx], G["fin"][idx] != 0,
                    np.zeros((B, 3)), np.zeros((B, 3)), 0.99)[2]
    Y = ag.fused_batch(6, (2 * B, 3)).double().numpy()[src]
    X = ag.fused_batch(0, (2 * B, D)).double().numpy()[src]
    np.testing.assert_allclose(X, G["online_X"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(Y, G["online_Y"], rtol=1e-4, atol=1e-4)
