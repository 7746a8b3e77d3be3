"""cn_actor_pop_pack and cn_actor_pop_forward against their statements (include/crowdnav.h), every comparison torch.equal:
member p's packed weights are the bytes cn_actor_pack_weights gives through the per-agent path (sync_fused_weights), and its
actions are the bits the solo cn_actor_forward call writes -- whatever the member's place, the number of members, their row counts
(tile edges, a member without rows, workgroups that leave early) and keys -- with the rows beyond n_p untouched.  One case is also
held to the float64 actor of tests/actor_f64.py within the bound that file derives, so that agreement with the solo kernel is not the
only evidence.  Then the Python layer: Population.act / agent.act_mfma share one noise series per agent, pack + forward capture into
one linear graph, and Population.actor_weights drives cn_actor_forward."""
import ctypes as C

import numpy as np
import pytest
import torch

import actor_f64 as A
from learner_handle import lib, stream
from td3_f64 import worst_ratio

pytestmark = pytest.mark.gpu

SENTINEL = -7.0                       # outside both action ranges
PAD = 16                              # rows behind every member's actions that no launch may touch
NS = (1, 16, 17, 33, 0, 5)            # one row, a full tile, a tile and a row, two tiles and a row, no tile, a ragged tile
SEEDS = (1, 0xD1B54A32D192ED03, 12345, (1 << 63) | 0x5DEECE66D, 7, 0)
COUNTERS = (1, 7, (1 << 32) + 5, (1 << 40) + 3, 2, 0)
SIGMAS = (0.1, 0.0, 1.0, 0.25, 0.1, 0.0)
MAX_VS = (0.22, 0.3, 0.22, 1.0, 0.5, 0.22)
MAX_WS = (2.0, 1.0, 0.5, 2.0, 3.0, 2.0)
CN_ERR_ARG = -1


def _f32(x):
    return float(np.float32(x))


def _actor(D, seed):
    from crowdnav.td3 import Actor
    torch.manual_seed(1000 + seed)
    return Actor(D, 2, 256).cuda()


def _perturb(actor, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(torch.randn(p.shape, generator=g, device="cuda") * 0.01)


class Solo:
    """The per-agent path for one actor: W^T staged and zero-padded, cn_actor_pack_weights twice, cn_actor_forward."""

    def __init__(self, actor):
        _abi, L = lib()
        D = actor.linear1.in_features
        Dp = (D + 31) // 32 * 32
        w1t = torch.zeros((Dp, 256), device="cuda")
        w1t[:D] = actor.linear1.weight.detach().t()
        w2t = actor.linear2.weight.detach().t().contiguous()
        self.w1p, self.w2p = torch.empty_like(w1t), torch.empty_like(w2t)
        _abi.check(L.cn_actor_pack_weights(C.c_void_p(w1t.data_ptr()), Dp, C.c_void_p(self.w1p.data_ptr()), 0, stream()))
        _abi.check(L.cn_actor_pack_weights(C.c_void_p(w2t.data_ptr()), 256, C.c_void_p(self.w2p.data_ptr()), 0, stream()))
        torch.cuda.synchronize()
        self.keep = actor
        self.w = _abi.CnActorWeights(w1p=self.w1p.data_ptr(), b1=actor.linear1.bias.data_ptr(), w2p=self.w2p.data_ptr(),
                                     b2=actor.linear2.bias.data_ptr(), w3=actor.linear3.weight.data_ptr(),
                                     b3=actor.linear3.bias.data_ptr(), obs_dim=D, obs_dim_padded=Dp, hidden=256, reserved=0)

    def forward(self, obs, n, max_v, max_w, sigma, seed, counter, w=None):
        _abi, L = lib()
        out = torch.full((n + PAD, 2), SENTINEL, device="cuda")
        _abi.check(L.cn_actor_forward(C.byref(self.w if w is None else w), C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), n,
                                      max_v, max_w, sigma, seed, counter, 0, stream()))
        torch.cuda.synchronize()
        return out


class Member:
    def __init__(self, actor, n, seed, counter, sigma, max_v, max_w, obs_seed):
        self.actor, self.n, self.seed, self.counter = actor, n, seed, counter
        self.sigma, self.max_v, self.max_w = _f32(sigma), _f32(max_v), _f32(max_w)
        D = actor.linear1.in_features
        self.obs = torch.randn((n, D), generator=torch.Generator().manual_seed(obs_seed)).cuda()
        self.out = torch.full((n + PAD, 2), SENTINEL, device="cuda")

    def struct(self):
        from crowdnav import _abi
        from crowdnav._fused import mlp_of
        return _abi.CnActorPopMember(actor=mlp_of(self.actor), obs=self.obs.data_ptr() if self.n else None, action=self.out.data_ptr(),
                                     n=self.n, reserved=0, max_v=self.max_v, max_w=self.max_w, sigma=self.sigma, reserved_f=0.0,
                                     seed=self.seed)

    def solo(self, add_noise, solo=None):
        if self.n == 0:       # an empty tensor has no address and cn_actor_forward refuses NULL: the solo call of no rows writes nothing
            return torch.full((PAD, 2), SENTINEL, device="cuda")
        return (solo or Solo(self.actor)).forward(self.obs, self.n, self.max_v, self.max_w, self.sigma if add_noise else 0.0,
                                                 self.seed, self.counter)


def _handle(members):
    from crowdnav._fused import FusedPopulationActor
    D = members[0].actor.linear1.in_features
    return FusedPopulationActor([m.struct() for m in members], D, torch.device("cuda:0"), 0, keep=members)


def _run(members, add_noise, handle=None):
    """pack + forward of `members` in one handle; returns each member's whole action buffer (padding included)."""
    h = handle or _handle(members)
    for m in members:
        m.out.fill_(SENTINEL)
    h.pack()
    h.forward([m.counter for m in members], add_noise)
    torch.cuda.synchronize()
    return [m.out.clone() for m in members]


@pytest.mark.parametrize("P", (1, 3))
@pytest.mark.parametrize("D", (1, 32, 33, 398, 1035))
def test_pack_is_sync_fused_weights_byte_for_byte(D, P):
    from crowdnav.td3 import Agent
    agents = [Agent(obs_dim=D, device="cuda:0", seed=10 * D + p, memory_size=16, batch_size=8) for p in range(P)]
    members = [Member(a.actor, 0, p, 0, 0.0, 0.22, 2.0, p) for p, a in enumerate(agents)]
    h = _handle(members)
    Dp = (D + 31) // 32 * 32
    for round_ in range(2):
        views = [h.packed(p) for p in range(P)]
        for w1p, w2p in views:
            assert w1p.shape == (Dp, 256) and w2p.shape == (256, 256)
            w1p.fill_(float("nan")); w2p.fill_(float("nan"))
        h.pack()
        torch.cuda.synchronize()
        for p, (a, (w1p, w2p)) in enumerate(zip(agents, views)):
            a.sync_fused_weights()
            torch.cuda.synchronize()
            assert a._fw["w1p"].shape == w1p.shape
            assert torch.equal(w1p, a._fw["w1p"]), (D, P, p, round_, "w1p")
            assert torch.equal(w2p, a._fw["w2p"]), (D, P, p, round_, "w2p")
            assert int((w1p == 0).sum()) >= (Dp - D) * 256           # the zero rows are written, not left as NaN
        for p in range(1, P):
            assert not torch.equal(views[0][0], views[p][0])        # distinct members
        for p, a in enumerate(agents):                              # ... then the weights move in place and are packed again
            _perturb(a.actor, 77 + p)
    w = h.weights(P - 1)
    assert (w.obs_dim, w.obs_dim_padded, w.hidden) == (D, Dp, 256)
    assert w.b1 == agents[-1].actor.linear1.bias.data_ptr() and w.w3 == agents[-1].actor.linear3.weight.data_ptr()


@pytest.fixture(scope="module")
def six():
    """D -> the six members of NS with distinct actors, keys and head ranges, and each member's Solo (packed once, shared)."""
    cache = {}

    def get(D):
        if D not in cache:
            ms = [Member(_actor(D, 10 * D + p), NS[p], SEEDS[p], COUNTERS[p], SIGMAS[p], MAX_VS[p], MAX_WS[p], 100 * D + p) for p in range(6)]
            cache[D] = (ms, [Solo(m.actor) for m in ms])
        return cache[D]
    return get


@pytest.mark.parametrize("add_noise", (0, 1))
@pytest.mark.parametrize("D", (1, 33, 398, 1035))          # Dp 32: one block; 64: even; 416: odd block count; 1056: three staging chunks
def test_forward_is_the_solo_call_bit_for_bit(six, D, add_noise):
    members, solos = six(D)
    got = _run(members, add_noise)
    for p, (m, s, g) in enumerate(zip(members, solos, got)):
        want = m.solo(add_noise, s)
        assert torch.equal(g, want), (D, add_noise, p, m.n)
        assert bool((g[m.n:] == SENTINEL).all()) and g[m.n:].shape[0] == PAD          # nothing beyond n_p
        assert bool((g[:m.n] != SENTINEL).all())
        assert bool((g[:m.n, 0] >= 0).all() and (g[:m.n, 0] <= m.max_v).all() and (g[:m.n, 1].abs() <= m.max_w).all())
    if add_noise:       # the members' noise is on where sigma > 0 and differs from the noiseless actions there
        quiet = _run(members, 0)
        for m, g, q in zip(members, got, quiet):
            assert torch.equal(g, q) == (m.sigma == 0.0 or m.n == 0)


@pytest.mark.parametrize("add_noise", (0, 1))
def test_forward_against_the_float64_actor(six, add_noise):
    """D = 398: every member within tests/actor_f64.py's bound of the float64 actor and its documented noise."""
    members, _ = six(398)
    got = _run(members, add_noise)
    worst = 0.0
    for m, g in zip(members, got):
        if m.n == 0:
            continue
        a = m.actor
        p = {k: v.detach().double() for k, v in (("w1", a.linear1.weight), ("b1", a.linear1.bias), ("w2", a.linear2.weight),
                                                 ("b2", a.linear2.bias), ("w3", a.linear3.weight), ("b3", a.linear3.bias))}
        want, bound = A.act(p, m.obs.double(), m.max_v, m.max_w, m.sigma if add_noise else 0.0, m.seed, m.counter)
        r = worst_ratio(g[:m.n], want, bound)
        assert torch.isfinite(g[:m.n]).all() and r <= 1.0, (m.n, r)
        worst = max(worst, r)
    print("cn_actor_pop_forward D 398 add_noise %d: worst error / bound %.3g" % (add_noise, worst))


def test_a_member_does_not_depend_on_its_place_or_its_neighbours():
    D = 398
    x = Member(_actor(D, 1), 21, 99, 5, 0.5, 0.22, 2.0, 1)
    want = x.solo(1)
    outs = []
    for place in (0, 2, 4):
        others = [Member(_actor(D, 50 + 7 * place + i), (3, 40, 16, 1)[i], 200 + place + i, 9 + i, 0.3, 0.22, 2.0, 60 + i) for i in range(4)]
        ms = others[:place] + [x] + others[place:]
        assert len(ms) == 5 and ms[place] is x
        outs.append(_run(ms, 1)[place])
    for o in outs:
        assert torch.equal(o, want)
    # twins: equal in everything but their action buffers
    t1 = Member(x.actor, 21, 99, 5, 0.5, 0.22, 2.0, 1)
    t2 = Member(x.actor, 21, 99, 5, 0.5, 0.22, 2.0, 1)
    o1, o2 = _run([t1, t2], 1)
    assert torch.equal(o1, o2) and torch.equal(o1, want)
    # equal weights and observations, different seeds: different noise, equal without it
    t3 = Member(x.actor, 21, 100, 5, 0.5, 0.22, 2.0, 1)
    o1, o3 = _run([t1, t3], 1)
    assert not torch.equal(o1, o3) and torch.equal(o1, want)
    q1, q3 = _run([t1, t3], 0)
    assert torch.equal(q1, q3) and not torch.equal(q1, o1)
    # ... and different counters with one seed
    t4 = Member(x.actor, 21, 99, 6, 0.5, 0.22, 2.0, 1)
    o1, o4 = _run([t1, t4], 1)
    assert not torch.equal(o1, o4)


def test_all_members_empty_launches_nothing_and_live_handle_refusals():
    _abi, L = lib()
    D = 33
    ms = [Member(_actor(D, p), 0, p, 1, 0.1, 0.22, 2.0, p) for p in range(2)]
    got = _run(ms, 1)
    assert all(bool((g == SENTINEL).all()) for g in got)
    h = _handle([Member(_actor(D, 3), 4, 1, 1, 0.1, 0.22, 2.0, 3)])
    assert L.cn_actor_pop_members(h.h) == 1
    assert L.cn_actor_pop_forward(h.h, None, 1, stream()) == CN_ERR_ARG and b"counters" in L.cn_last_error()
    w = _abi.CnActorWeights()
    for member in (-1, 1, 64):
        assert L.cn_actor_pop_weights(h.h, member, C.byref(w)) == CN_ERR_ARG
        assert b"member %d" % member in L.cn_last_error() and b"out of range" in L.cn_last_error()
    assert not w.w1p
    assert L.cn_actor_pop_weights(h.h, 0, None) == CN_ERR_ARG and b"out" in L.cn_last_error()
    torch.cuda.synchronize()


def _agents(P, D=398, sigma=0.5, device="cuda:0"):
    from crowdnav.td3 import Agent
    ags = [Agent(obs_dim=D, device=device, seed=40 + p, memory_size=16, batch_size=8, explore_sigma=sigma) for p in range(P)]
    return ags


def test_population_act_and_act_mfma_share_one_noise_series():
    from crowdnav.td3 import Population
    P, D, n = 2, 398, 20
    agents, twins = _agents(P), _agents(P)
    for a, t in zip(agents, twins):
        assert all(torch.equal(x, y) for x, y in zip(a.actor.parameters(), t.actor.parameters())) and a.noise_state() == t.noise_state()
    obs = [torch.randn((n, D), generator=torch.Generator().manual_seed(p)).cuda() for p in range(P)]
    out = [torch.zeros((n, 2), device="cuda") for _ in range(P)]
    pop = Population(agents)
    with pytest.raises(RuntimeError, match="bind_act"):
        pop.act()
    pop.bind_act(obs, out)
    for call in range(2):
        res = pop.act()
        torch.cuda.synchronize()
        for p in range(P):
            assert res[p] is out[p]
            assert torch.equal(out[p], twins[p].act_mfma(obs[p])), (call, p)
    for p in range(P):
        assert torch.equal(agents[p].act_mfma(obs[p]), twins[p].act_mfma(obs[p]))
        assert agents[p].noise_state() == twins[p].noise_state() and agents[p].noise_state()[1] == 3
    # add_noise=False advances the counter too (as act_mfma), and a restored noise state carries over to the population's launch
    pop.act(add_noise=False)
    for p in range(P):
        assert torch.equal(out[p], twins[p].act_mfma(obs[p], add_noise=False))
    for a, t in zip(agents, twins):
        a.set_noise_state(1234567, 41); t.set_noise_state(1234567, 41)
    pop.act()
    torch.cuda.synchronize()
    for p in range(P):
        assert torch.equal(out[p], twins[p].act_mfma(obs[p])) and agents[p].noise_state() == (1234567, 42)


def test_actor_weights_hand_off_to_cn_actor_forward():
    from crowdnav.td3 import Population
    P, D, n = 3, 33, 18
    agents = _agents(P, D, device="cuda")         # (agents on "cuda", buffers on "cuda:0": one device)
    obs = [torch.randn((n, D), generator=torch.Generator().manual_seed(p)).cuda() for p in range(P)]
    out = [torch.full((n + PAD, 2), SENTINEL, device="cuda")[:n] for _ in range(P)]
    pop = Population(agents).bind_act(obs, out)
    pop.act()
    torch.cuda.synchronize()
    for p, a in enumerate(agents):
        w = pop.actor_weights(p)
        seed, calls = a.noise_state()
        want = Solo(a.actor).forward(obs[p], n, a.max_v, a.max_w, a.explore_sigma, seed, calls)
        got = Solo(a.actor).forward(obs[p], n, a.max_v, a.max_w, a.explore_sigma, seed, calls, w=w)
        assert torch.equal(got, want) and torch.equal(out[p], want[:n]), p


def test_pack_and_forward_capture_into_one_linear_graph():
    D = 398
    ms = [Member(_actor(D, 20 + p), (17, 5, 32)[p], 300 + p, 11 + p, 0.2, 0.22, 2.0, 30 + p) for p in range(3)]
    h = _handle(ms)
    before = _run(ms, 1, h)                       # warm-up outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                     # one stream: pack, then forward -- a chain, no parallel branches
        h.pack()
        h.forward([m.counter for m in ms], True)
    for p, m in enumerate(ms):
        _perturb(m.actor, 500 + p)
    torch.cuda.synchronize()
    for replay in range(2):
        for m in ms:
            m.out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for p, m in enumerate(ms):
            want = m.solo(1)                      # packed afresh from the changed weights by the per-agent path
            assert torch.equal(m.out, want), (replay, p)
            assert not torch.equal(m.out, before[p])
