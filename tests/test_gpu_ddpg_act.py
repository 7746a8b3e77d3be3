"""cn_ddpg_act (csrc/crowdnav_ddpg.hip) on the device: DDPG's actor with the reference's Ornstein-Uhlenbeck noise in one launch.
Everything is bit equality: the process against the reference's recorded one (tests/golden/ddpg.npz: ou_u, ou_x, ou_reset_at), the
action against act_mfma's head value plus OUNoise.sample's state in float64, the device draw against tests/ou_ref.py; then
Agent.act_ou_fused / bind_act_ou_fused against the PyTorch path, and the trainer's --ou-act."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ou_ref
from learner_handle import lib, stream

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ddpg.npz"))
CANARY = -77.25
DEV = "cuda"


def _agent(obs_dim, n, seed=2, heads=0.2):
    """A DDPG agent on the device whose heads are spread over their ranges (linear3 from U(+-heads) instead of 3e-3), packed."""
    from crowdnav.ddpg import Agent
    ag = Agent(obs_dim=obs_dim, n_envs=n, device=DEV, seed=seed, memory_size=16)
    with torch.no_grad():
        g = torch.Generator(device=DEV).manual_seed(seed + 100)
        for p in (ag.actor.linear3.weight, ag.actor.linear3.bias):
            p.copy_((torch.rand(p.shape, generator=g, device=DEV) * 2 - 1) * heads)
    ag.sync_fused_weights()
    return ag


def _f64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), device=DEV).contiguous()


def ddpg_act(ag, obs, state, n=None, reset=None, u=None, sigma=0.2, add_noise=1, seed=5, counter=9, action=None, noise_out=None,
             mu=0.0, theta=0.15):
    """One raw cn_ddpg_act call on torch's current stream, synchronised; returns the action buffer."""
    _abi, L = lib()
    n = obs.shape[0] if n is None else n
    if action is None:
        action = torch.full((obs.shape[0], 2), CANARY, dtype=torch.float32, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    io = _abi.CnDdpgActIO(obs=obs.data_ptr(), state=ptr(state), reset=ptr(reset), u=ptr(u), action=action.data_ptr(),
                          noise_out=ptr(noise_out), mu=mu, theta=theta, sigma=sigma, seed=seed, counter=counter,
                          max_v=ag.max_v, max_w=ag.max_w, n=n, add_noise=add_noise)
    rc = L.cn_ddpg_act(C.byref(ag._fw_struct), C.byref(io), 0, stream())
    assert rc == 0, L.cn_last_error()
    torch.cuda.synchronize()
    return action


def _clip(ag, a):
    return torch.max(torch.min(a, ag._hi), ag._lo)


# ---- reference parity of the process ---------------------------------------------------------------------------------------------

def test_one_row_follows_the_references_recorded_process():
    ag = _agent(46, 1)
    obs = torch.zeros((1, 46), device=DEV)
    u, want, at = G["ou_u"], G["ou_x"], int(G["ou_reset_at"])
    state = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    reset = torch.zeros(1, dtype=torch.uint8, device=DEV)
    for k in range(u.shape[0]):
        reset[0] = 1 if k == at else 0
        ddpg_act(ag, obs, state, reset=reset, u=_f64(u[k:k + 1]))
        assert np.array_equal(state.cpu().numpy()[0], want[k]), k


def test_three_rows_with_their_own_reset_calls():
    ag = _agent(46, 3)
    obs = torch.zeros((3, 46), device=DEV)
    u, want, at = G["ou_u"], G["ou_x"], int(G["ou_reset_at"])
    other = at + 3                                           # row 1's episode ends at another call
    state = torch.zeros((3, 2), dtype=torch.float64, device=DEV)
    ref = np.zeros((3, 2))
    for k in range(u.shape[0]):
        mask = np.array([k == at, k == other, k == at])
        uk = np.repeat(u[k:k + 1], 3, axis=0)
        ddpg_act(ag, obs, state, reset=torch.as_tensor(mask.astype(np.uint8), device=DEV), u=_f64(uk))
        ref = ou_ref.update(ref, uk, reset=mask)
        got = state.cpu().numpy()
        assert np.array_equal(got[0], want[k]) and np.array_equal(got[2], want[k]), k
        assert np.array_equal(got, ref), k
        assert np.array_equal(got[1], want[k]) == (k < at), k     # row 1 leaves the recorded process where the others are reset


# ---- the whole action ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 16, 17, 33])
@pytest.mark.parametrize("obs_dim", [363, 46])
def test_action_is_the_mfma_head_plus_the_float64_noise_clipped(obs_dim, n):
    _check_action(obs_dim, n)


def test_action_where_the_tile_needs_more_than_64_kib_of_lds():
    """800 inputs: 16 x (801 + 257) floats = 66 KiB, the launch that raises the kernel's dynamic-LDS limit first."""
    _check_action(800, 17)


def _check_action(obs_dim, n):
    """Three calls per shape; row e's state on call c starts below, inside or above what the clips let through ((e + c) % 3), so
    every row meets the lower clip, no clip and the upper clip of both components."""
    from crowdnav.ddpg import OUNoise
    ag = _agent(obs_dim, n)
    g = torch.Generator(device=DEV).manual_seed(n * 1000 + obs_dim)
    obs = torch.randn((n, obs_dim), generator=g, device=DEV)
    pi = ag.act_mfma(obs, add_noise=False)
    assert float(pi[:, 0].min()) >= 0 and float(pi[:, 0].max()) <= ag.max_v and float(pi[:, 1].abs().max()) <= ag.max_w
    seen = set()
    for c in range(3):
        kind = (torch.arange(n, device=DEV) + c) % 3 - 1                                   # -1, 0, 1
        jitter = torch.rand((n, 2), generator=g, dtype=torch.float64, device=DEV) * 0.01
        state = (kind[:, None].double() * torch.tensor([0.7, 5.0], dtype=torch.float64, device=DEV) + jitter).contiguous()
        state[kind == 0] = jitter[kind == 0] * torch.tensor([1.0, 10.0], dtype=torch.float64, device=DEV) - 0.05
        u = torch.rand((n, 2), generator=g, dtype=torch.float64, device=DEV)
        reset = (torch.arange(n, device=DEV) % 5 == 4).to(torch.uint8) if c == 2 else None
        twin = OUNoise(n, device=DEV)
        twin.state, twin.sigma = state.clone(), 0.17
        if reset is not None:
            twin.reset(reset)
        x1 = twin.sample(0, u=u)
        assert np.array_equal(x1.cpu().numpy(), ou_ref.update(state.cpu().numpy(), u.cpu().numpy(), sigma=0.17,
                                                               reset=None if reset is None else reset.cpu().numpy()))
        raw = (pi.double() + x1).float()
        want = _clip(ag, raw)
        action = ddpg_act(ag, obs, state, reset=reset, u=u, sigma=0.17)
        assert torch.equal(state, x1)
        assert torch.equal(action, want)
        assert np.array_equal(action.cpu().numpy(), ou_ref.action(pi.cpu().numpy(), x1.cpu().numpy(), ag.max_v, ag.max_w))
        for o in (0, 1):
            seen |= {(o, "lo")} if bool((raw[:, o] < ag._lo[o]).any()) else set()
            seen |= {(o, "hi")} if bool((raw[:, o] > ag._hi[o]).any()) else set()
            seen |= {(o, "in")} if bool(((raw[:, o] > ag._lo[o]) & (raw[:, o] < ag._hi[o])).any()) else set()
    assert seen == {(o, k) for o in (0, 1) for k in ("lo", "hi", "in")}, seen


# ---- the device draw -------------------------------------------------------------------------------------------------------------

def test_the_device_draw_is_the_documented_one_and_knows_nothing_of_n():
    ag = _agent(46, 33)
    g = torch.Generator(device=DEV).manual_seed(4)
    obs = torch.randn((33, 46), generator=g, device=DEV)
    seed, got = 0x9E3779B97F4A7C15 ^ 0x1234, {}
    for n, counter in ((17, 3), (33, 3), (33, 4)):
        state = torch.zeros((33, 2), dtype=torch.float64, device=DEV)
        ddpg_act(ag, obs, state, n=n, seed=seed, counter=counter)
        got[n, counter] = state.cpu().numpy()
        want = ou_ref.update(np.zeros((n, 2)), ou_ref.draws(seed, counter, n))
        assert np.array_equal(got[n, counter][:n], want), (n, counter)
        assert not got[n, counter][n:].any()
    assert np.array_equal(got[17, 3][:17], got[33, 3][:17])
    assert not (got[33, 3] == got[33, 4]).any()
    # from a state that is not mu, with theta's pull: the draw is still the update's U
    state = torch.full((33, 2), 0.4, dtype=torch.float64, device=DEV)
    ddpg_act(ag, obs, state, seed=seed, counter=8, sigma=0.3, mu=0.1, theta=0.25)
    assert np.array_equal(state.cpu().numpy(), ou_ref.update(np.full((33, 2), 0.4), ou_ref.draws(seed, 8, 33), mu=0.1, theta=0.25, sigma=0.3))


# ---- rows and flags --------------------------------------------------------------------------------------------------------------

def test_rows_beyond_n_are_untouched_and_noise_out_is_the_state():
    ag = _agent(363, 40)
    g = torch.Generator(device=DEV).manual_seed(6)
    obs = torch.randn((40, 363), generator=g, device=DEV)
    n = 17
    state = torch.full((40, 2), CANARY, dtype=torch.float64, device=DEV)
    state[:n] = 0.25
    noise_out = torch.full((40, 2), CANARY, dtype=torch.float64, device=DEV)
    u = torch.rand((40, 2), generator=g, dtype=torch.float64, device=DEV)
    action = ddpg_act(ag, obs, state, n=n, u=u, noise_out=noise_out)
    for t in (state, noise_out, action):
        assert bool((t[n:] == CANARY).all()) and not bool((t[:n] == CANARY).any())
    assert torch.equal(noise_out[:n], state[:n])
    assert np.array_equal(state[:n].cpu().numpy(), ou_ref.update(np.full((n, 2), 0.25), u[:n].cpu().numpy()))


def test_add_noise_zero_is_the_deterministic_policy_and_leaves_the_state():
    ag = _agent(363, 33)
    g = torch.Generator(device=DEV).manual_seed(7)
    obs = torch.randn((33, 363), generator=g, device=DEV)
    state = torch.rand((33, 2), generator=g, dtype=torch.float64, device=DEV)
    before = state.clone()
    noise_out = torch.full((33, 2), CANARY, dtype=torch.float64, device=DEV)
    reset = torch.ones(33, dtype=torch.uint8, device=DEV)
    action = ddpg_act(ag, obs, state, reset=reset, add_noise=0, noise_out=noise_out)
    assert torch.equal(state, before) and bool((noise_out == CANARY).all())
    assert torch.equal(action, ag.act_mfma(obs, add_noise=False))
    assert torch.equal(ddpg_act(ag, obs, None, add_noise=0), action)            # no state needed


# ---- the Python layer ------------------------------------------------------------------------------------------------------------

def _pair(n, obs_dim=46, seed=3):
    a, b = _agent(obs_dim, n, seed=seed), _agent(obs_dim, n, seed=seed)
    for ag in (a, b):
        ag.noise.min_sigma, ag.noise.decay_period = 0.05, 4          # sigma moves with `step`
    shadow = torch.Generator(device=DEV).manual_seed(seed)           # OUNoise's own generator, step for step
    return a, b, shadow


def test_act_ou_fused_and_the_torch_path_keep_the_same_noise():
    n = 17
    a, b, shadow = _pair(n)
    g = torch.Generator(device=DEV).manual_seed(8)
    mask_prev = None
    for k in range(5):
        obs = torch.randn((n, 46), generator=g, device=DEV)
        u = torch.rand((n, 2), generator=shadow, dtype=torch.float64, device=DEV)
        act_a = a.act(obs, add_noise=True, step=k)
        act_b = b.act_ou_fused(obs, reset=mask_prev, step=k, u=u)
        assert a.noise.sigma == b.noise.sigma and (k == 0 or a.noise.sigma < 0.2)
        assert torch.equal(a.noise.state, b.noise.state), k                     # the noise term, exactly
        want = _clip(b, (b.act_mfma(obs, add_noise=False).double() + b.noise.state).float())
        assert torch.equal(act_b, want), k
        torch.testing.assert_close(act_a, act_b, rtol=0, atol=1e-5)             # the eager actor against the MFMA actor
        mask_prev = (torch.arange(n, device=DEV) % 4 == k % 4).to(torch.uint8)  # a moving mask: the episodes that just ended
        a.reset_noise(mask_prev)
    assert float(b.noise.state.abs().max()) > 0
    with pytest.raises(ValueError, match="OU noise has 17 states for 5 observations"):
        b.act_ou_fused(torch.zeros((5, 46), device=DEV))


def test_the_two_paths_mix_call_by_call_on_one_state():
    n = 16
    a, m, shadow = _pair(n)
    g = torch.Generator(device=DEV).manual_seed(9)
    for k in range(6):
        obs = torch.randn((n, 46), generator=g, device=DEV)
        u = torch.rand((n, 2), generator=shadow, dtype=torch.float64, device=DEV)
        mask = (torch.arange(n, device=DEV) % 3 == k % 3)
        a.act(obs, add_noise=True, step=k)
        a.reset_noise(mask)
        if k % 2 == 0:
            m.act_ou_fused(obs, step=k, u=u)
            torch.rand((n, 2), generator=m.noise.gen, dtype=torch.float64, device=DEV)      # keep its own stream in step
            m.reset_noise(mask)                                                             # the torch path's reset on the fused path's state
        else:
            m.act(obs, add_noise=True, step=k)
            m.act_ou_fused(obs, reset=mask.to(torch.uint8), add_noise=False)                # (the deterministic call resets nothing)
            m.reset_noise(mask)
        assert torch.equal(a.noise.state, m.noise.state) and a.noise.sigma == m.noise.sigma, k


def test_bound_call_replayed_from_a_graph_equals_the_eager_calls():
    n = 33
    a, b, _ = _pair(n, obs_dim=363)
    for ag in (a, b):
        ag.noise.min_sigma = ag.noise.max_sigma                      # a captured call keeps its sigma: a constant one
    g = torch.Generator(device=DEV).manual_seed(10)
    obs = torch.zeros((n, 363), device=DEV)
    out = torch.zeros((n, 2), device=DEV)
    reset = torch.zeros(n, dtype=torch.uint8, device=DEV)
    u = torch.zeros((n, 2), dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call = a.bind_act_ou_fused(obs, out, reset, u=u)             # bound to the stream it will be captured on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    assert not bool(a.noise.state.any())                             # capturing ran nothing
    for k in range(3):
        obs.copy_(torch.randn((n, 363), generator=g, device=DEV))
        u.copy_(torch.rand((n, 2), generator=g, dtype=torch.float64, device=DEV))
        reset.copy_((torch.arange(n, device=DEV) % 3 == k).to(torch.uint8))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = b.act_ou_fused(obs, reset=reset, u=u)
        assert torch.equal(out, want) and torch.equal(a.noise.state, b.noise.state), k
    assert float(a.noise.state.abs().max()) > 0


# ---- the trainer -----------------------------------------------------------------------------------------------------------------

def test_trainer_ou_act_fused_makes_no_torch_act_and_torch_makes_them(tmp_path, monkeypatch):
    from crowdnav import ddpg, train
    calls = {"act": 0, "reset_noise": 0, "act_ou_fused": 0}
    for name in calls:
        orig = getattr(ddpg.Agent, name)

        def counted(self, *a, _orig=orig, _key=name, **kw):
            calls[_key] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(ddpg.Agent, name, counted)
    for mode in ("fused", "torch"):
        before = dict(calls)
        agent, episodes = train.main(["--algo", "ddpg", "--learner", "fused", "--ou-noise", "--ou-act", mode, "--envs", "64", "--launches", "120",
                                      "--max-steps", "25", "--scenario", "bench", "--memory", "20000", "--log-every", "60",
                                      "--out", str(tmp_path / mode)])
        torch.cuda.synchronize()
        made = {k: calls[k] - before[k] for k in calls}
        assert isinstance(agent, ddpg.Agent) and episodes > 64
        assert all(bool(torch.isfinite(p).all()) for m in (agent.actor, agent.critic, agent.actor_t, agent.critic_t) for p in m.parameters())
        assert agent.noise.state.shape == (64, 2) and float(agent.noise.state.abs().max()) > 0
        if mode == "fused":
            assert made == {"act": 0, "reset_noise": 0, "act_ou_fused": 120}, made
        else:
            assert made == {"act": 120, "reset_noise": 120, "act_ou_fused": 0}, made
