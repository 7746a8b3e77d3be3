"""cn_td3_pop_update (include/crowdnav.h: a population of TD3 learners in the launches of one) against its statement: member p equals
a solo cn_td3_update handle made from cfgs[p] and given the same do_actor sequence -- the six networks, the loss and the gathered
batch, by torch.equal, after every one of four updates (do_actor 0, 1, 0, 1).  No tolerance anywhere in this file.
Shapes (obs_dim, hidden, batch, P): the smallest that cross each tile of the GEMM launches (F 16 x 16, G 16 x 32, H 32 x 32, the q and
da partial-sum tiles), and the product shape at P = 2."""
import ctypes as C

import pytest
import torch

from learner_handle import LearnerHandle, alias, err, lib, ring_fields, stream

pytestmark = pytest.mark.gpu

DO_ACTOR = (0, 1, 0, 1)
NETS = ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t")
SHAPES = [(45, 33, 40, 3), (1, 17, 33, 2), (30, 16, 17, 5), (20, 48, 129, 2), (45, 1, 3, 4), (398, 256, 128, 2), (45, 33, 40, 1)]
CN_ERR_ARG, CN_ERR_CONFIG = -1, -2


class Member:
    """What one learner is made from, on the host: its hyper-parameters, its six networks (targets = copies, as Agent makes them), its
    ring of seeded random rows and the ring's live size.  instance() puts a fresh copy of all of it on the device."""

    def __init__(self, D, H, B, key, seed=None, lr_actor=3e-4, lr_critic=3e-4, gamma=0.99, noise_std=0.2, noise_clip=0.5, live=300, cap=None,
                 **shared):
        g = torch.Generator().manual_seed(1000 + key)
        self.D, self.H, self.B = D, H, B
        self.hyper = dict(policy_delay=2, tau=0.005, beta1=0.9, beta2=0.999, eps=1e-8, max_v=0.22, max_w=2.0)
        self.hyper.update(shared)
        self.hyper.update(gamma=gamma, lr_actor=lr_actor, lr_critic=lr_critic, noise_std=noise_std, noise_clip=noise_clip)
        self.seed = (0x9E3779B97F4A7C15 * (key + 1)) & 0xFFFFFFFFFFFFFFFF if seed is None else seed

        def mlp(n_in, n_out):
            return [torch.randn(s, generator=g) * 0.2 for s in ((H, n_in), (H,), (H, H), (H,), (n_out, H), (n_out,))]
        actor, q1, q2 = mlp(D, 2), mlp(D + 2, 1), mlp(D + 2, 1)
        self.nets = dict(actor=actor, actor_t=[t.clone() for t in actor], q1=q1, q1_t=[t.clone() for t in q1], q2=q2, q2_t=[t.clone() for t in q2])
        cap = cap if cap is not None else max(live, 1)
        self.ring = dict(s=torch.randn((cap, D), generator=g), a=torch.rand((cap, 2), generator=g), r=torch.randn(cap, generator=g),
                         s2=torch.randn((cap, D), generator=g), d=(torch.rand(cap, generator=g) < 0.1).float())
        self.live = live

    def instance(self):
        return Instance(self)


class Instance:
    """A member's state on the device and the cn_td3_config that points at it."""

    def __init__(self, m):
        _abi, _ = lib()
        self.m = m
        self.nets = {k: [t.cuda().contiguous() for t in ts] for k, ts in m.nets.items()}
        self.ring = {k: t.cuda().contiguous() for k, t in m.ring.items()}
        self.size = torch.tensor([m.live], dtype=torch.int64, device="cuda")
        mlps = {k: _abi.CnTd3Mlp(*[t.data_ptr() for t in ts]) for k, ts in self.nets.items()}
        self.cfg = _abi.CnTd3Config(obs_dim=m.D, hidden=m.H, batch=m.B, reserved=0.0, seed=m.seed, **ring_fields(dict(self.ring, size=self.size)),
                                    **m.hyper, **mlps)

    def params(self):
        return [t.clone() for k in NETS for t in self.nets[k]]

    def batch_shapes(self):
        B, Dc = self.m.B, self.m.D + 2
        return ((B, Dc), (B, Dc), (B,), (B,), (B, 2))


def _snapshot(inst, loss, batch_ptr):
    """(the 36 parameter tensors, the loss, the five gathered buffers) of one learner, after a synchronisation."""
    out = inst.params() + [loss.clone()]
    for what, shape in enumerate(inst.batch_shapes()):
        ptr = batch_ptr(what)
        assert ptr, what
        out.append(alias(ptr, shape).clone())
    return out


def run_solo(member, mode=0, seq=DO_ACTOR):
    """A solo handle on a fresh instance of `member`: the snapshot after each update of `seq`."""
    inst = member.instance()
    h = LearnerHandle("td3", inst.cfg, inst)
    try:
        assert h.set_replay_sample(mode) == 0, err()
        loss = alias(h.L.cn_td3_loss_dev(h.h), ())
        snaps = []
        for a in seq:
            h.update(a)
            snaps.append(_snapshot(inst, loss, lambda what: h.L.cn_td3_batch_dev(h.h, what)))
        return snaps
    finally:
        h.close()


class Pop:
    def __init__(self, members, mode=0):
        _abi, L = lib()
        self.L, self.insts = L, [m.instance() for m in members]
        self.P = len(members)
        self.cfgs = (_abi.CnTd3Config * self.P)(*[i.cfg for i in self.insts])
        self.h = C.c_void_p()
        assert L.cn_td3_pop_create(self.cfgs, self.P, 0, C.byref(self.h)) == 0, err()
        assert L.cn_td3_pop_members(self.h) == self.P
        if mode:
            assert L.cn_td3_pop_set_replay_sample(self.h, mode) == 0, err()
        self.loss = alias(L.cn_td3_pop_loss_dev(self.h), (self.P,))

    def update(self, a):
        assert self.L.cn_td3_pop_update(self.h, a, stream()) == 0, err()

    def snapshot(self):
        torch.cuda.synchronize()
        return [_snapshot(inst, self.loss[p], lambda what, p=p: self.L.cn_td3_pop_batch_dev(self.h, p, what)) for p, inst in enumerate(self.insts)]

    def close(self):
        if self.h:
            self.L.cn_td3_pop_destroy(self.h)
            self.h = None


def run_pop(members, mode=0, seq=DO_ACTOR):
    """-> snaps[update][member]"""
    pop = Pop(members, mode)
    try:
        snaps = []
        for a in seq:
            pop.update(a)
            snaps.append(pop.snapshot())
        return snaps
    finally:
        pop.close()


def _same(got, want, where):
    assert len(got) == len(want) == 36 + 1 + 5
    for j, (g, w) in enumerate(zip(got, want)):
        name = "%s[%d]" % (NETS[j // 6], j % 6) if j < 36 else "loss" if j == 36 else "batch_dev %d" % (j - 37)
        assert g.shape == w.shape and torch.equal(g, w), (where, name, float((g - w).abs().max()))
        assert torch.isfinite(g).all(), (where, name)


def _members(D, H, B, P, live=300):
    """P members that differ in everything a member may differ in."""
    return [Member(D, H, B, key=p, lr_actor=3e-4 * (1 + p), lr_critic=1e-3 / (1 + p), gamma=0.99 - 0.02 * p, noise_std=0.2 + 0.05 * p,
                   noise_clip=0.5 - 0.05 * p, live=live + 7 * p) for p in range(P)]


@pytest.mark.parametrize("D,H,B,P", SHAPES)
def test_every_member_equals_its_solo_handle(D, H, B, P):
    members = _members(D, H, B, P)
    got = run_pop(members)
    for p, m in enumerate(members):
        want = run_solo(m)
        for u in range(len(DO_ACTOR)):
            _same(got[u][p], want[u], (D, H, B, P, "member %d" % p, "update %d" % u))
        assert not torch.equal(want[0][17], want[-1][17])      # q1's b3 moved (its gradient is the sum of dq)


@pytest.mark.parametrize("mode", (0, 1))
def test_varied_members_and_live_sizes_in_both_sample_modes(mode):
    """Seeds, learning rates, gamma and the noise parameters differ; the rings hold fewer rows than the batch, exactly a batch, and
    a few thousand."""
    D, H, B = 45, 33, 40
    members = [Member(D, H, B, key=50 + p, lr_actor=3e-4 * (1 + p), lr_critic=1e-3 / (1 + p), gamma=0.99 - 0.02 * p, noise_std=0.2 + 0.05 * p,
                      noise_clip=0.5 - 0.05 * p, live=live) for p, live in enumerate((17, 40, 3001))]
    got = run_pop(members, mode)
    for p, m in enumerate(members):
        want = run_solo(m, mode)
        for u in range(len(DO_ACTOR)):
            _same(got[u][p], want[u], (mode, "member %d" % p, "update %d" % u))
    if mode == 1:                                  # the distinct draw: no ring row twice where the ring holds at least a batch
        for p in (1, 2):
            rows = got[-1][p][37][:, :D]
            assert len({tuple(r.tolist()) for r in rows}) == B, p


def test_a_member_does_not_depend_on_its_position_or_on_the_population_size():
    D, H, B = 45, 33, 40
    x = Member(D, H, B, key=7, lr_actor=1e-3, gamma=0.9, noise_std=0.3, live=77)
    fill = _members(D, H, B, 4)
    runs = [run_pop([x])[-1][0], run_pop(fill[:2] + [x])[-1][2], run_pop(fill + [x])[-1][4]]
    for r in runs[1:]:
        _same(r, runs[0], "position")


def test_members_do_not_interfere_and_twins_stay_twins():
    D, H, B = 30, 16, 17
    a, b = Member(D, H, B, key=1), Member(D, H, B, key=2)
    twin = Member(D, H, B, key=1)                  # a's configuration, parameters and ring, in separate device copies
    snaps = run_pop([a, b, twin, Member(D, H, B, key=3)])
    last = snaps[-1]
    _same(last[2], last[0], "twins")
    for p, q in ((0, 1), (0, 3), (1, 2), (1, 3), (2, 3)):
        for j in range(36):
            assert not torch.equal(last[p][j], last[q][j]), (p, q, j)


def test_captured_pair_replayed_twice_equals_four_eager_updates():
    D, H, B, P = 45, 33, 40, 3
    members = _members(D, H, B, P)
    want = run_pop(members)[-1]                    # (also loads the kernels before anything is captured)
    pop = Pop(members)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pop.update(0)
            pop.update(1)
        for _ in range(2):
            g.replay()
        got = pop.snapshot()
        for p in range(P):
            _same(got[p], want[p], "graph, member %d" % p)
        del g
    finally:
        pop.close()


def test_refusals():
    _abi, L = lib()
    D, H, B = 20, 16, 8
    h = C.c_void_p()

    def create(insts, n=None):
        cfgs = (_abi.CnTd3Config * len(insts))(*[i.cfg for i in insts])
        rc = L.cn_td3_pop_create(cfgs, len(insts) if n is None else n, 0, C.byref(h))
        assert not h.value
        return rc, err()

    base = [Member(D, H, B, key=p).instance() for p in range(3)]
    for n in (0, -1, 65):
        rc, msg = create(base, n)
        assert rc == CN_ERR_ARG and "n_members" in msg, (n, rc, msg)
    assert L.cn_td3_pop_create(None, 1, 0, C.byref(h)) == CN_ERR_ARG and "null" in err()
    # every shared field, at member 2
    for field, val in (("obs_dim", D + 1), ("hidden", H + 1), ("batch", B + 1), ("policy_delay", 3), ("beta1", 0.8), ("beta2", 0.99),
                       ("eps", 1e-7), ("tau", 0.01), ("max_v", 0.3), ("max_w", 1.0)):
        insts = [Member(D, H, B, key=p).instance() for p in range(3)]
        setattr(insts[2].cfg, field, val)
        rc, msg = create(insts)
        assert rc == CN_ERR_CONFIG and "member 2" in msg and field in msg, (field, rc, msg)
    # what members may differ in is not refused (checked by the equality tests); a null network pointer, no ring
    insts = [Member(D, H, B, key=p).instance() for p in range(2)]
    insts[1].cfg.q2_t.w2 = None
    rc, msg = create(insts)
    assert rc == CN_ERR_ARG and "member 1" in msg and "null parameter pointer" in msg, (rc, msg)
    for field in ("replay_s", "replay_size_dev"):
        insts = [Member(D, H, B, key=p).instance() for p in range(2)]
        setattr(insts[1].cfg, field, None)
        rc, msg = create(insts)
        assert rc == CN_ERR_ARG and "member 1" in msg and "no replay ring" in msg, (field, rc, msg)
    # two members naming one parameter tensor
    insts = [Member(D, H, B, key=p).instance() for p in range(3)]
    insts[2].cfg.q1.b2 = insts[0].cfg.q1.b2
    rc, msg = create(insts)
    assert rc == CN_ERR_CONFIG and "same parameter tensor" in msg and "members 0" in msg and "and 2" in msg, (rc, msg)
    # the handle's calls
    assert L.cn_td3_pop_update(None, 0, stream()) == CN_ERR_ARG and "null handle" in err()
    assert L.cn_td3_pop_set_replay_sample(None, 0) == CN_ERR_ARG and "null handle" in err()
    assert L.cn_td3_pop_members(None) == 0 and not L.cn_td3_pop_loss_dev(None) and not L.cn_td3_pop_batch_dev(None, 0, 0)
    members = [Member(D, H, B, key=p, live=500) for p in range(2)]
    pop = Pop(members, mode=1)
    try:
        for member, what in ((-1, 0), (2, 0), (0, -1), (0, 5)):
            assert not L.cn_td3_pop_batch_dev(pop.h, member, what), (member, what)
        for bad in (2, -1):
            assert L.cn_td3_pop_set_replay_sample(pop.h, bad) == CN_ERR_ARG and "cn_td3_pop_set_replay_sample" in err() and "mode" in err()
        pop.update(0)                              # still mode 1
        got = pop.snapshot()
        for p, m in enumerate(members):
            _same(got[p], run_solo(m, 1, (0,))[0], "mode kept, member %d" % p)
            assert not torch.equal(got[p][37], run_solo(m, 0, (0,))[0][37])
    finally:
        pop.close()


def test_python_population_follows_policy_delay_and_returns_fresh_losses():
    """crowdnav.td3.Population over two Agents: learn(step) is the members' Agent._fused_learn(step), losses [P] in a tensor of its own."""
    from crowdnav import td3

    def agents():
        out = []
        for p in range(2):
            a = td3.Agent(obs_dim=20, hidden=32, batch_size=16, memory_size=64, device="cuda:0", seed=3 + p, gamma=0.99 - 0.01 * p)
            g = torch.Generator().manual_seed(p)
            n = 40
            a.memory.add(torch.randn((n, 20), generator=g).cuda(), torch.rand((n, 2), generator=g).cuda(), torch.randn(n, generator=g).cuda(),
                         torch.randn((n, 20), generator=g).cuda(), (torch.rand(n, generator=g) < 0.1).cuda())
            out.append(a)
        return out
    solo, mem = agents(), agents()
    for a in solo:
        a.enable_fused_update()
    pop = td3.Population(mem)
    assert len(pop) == 2 and pop.ready()
    losses = []
    for step in (1, 2, 3, 4):
        got = pop.learn(step)
        want = torch.stack([a.learn(step) for a in solo])
        torch.cuda.synchronize()
        assert got.shape == (2,) and torch.equal(got, want), step
        losses.append(got)
    assert losses[0].data_ptr() != losses[1].data_ptr() and not torch.equal(losses[0], losses[1])
    for a, b in zip(solo, mem):
        for net in ("actor", "actor_t", "q1", "q1_t", "q2", "q2_t"):
            for x, y in zip(getattr(a, net).parameters(), getattr(b, net).parameters()):
                assert torch.equal(x, y), net
    assert torch.equal(pop.batch_dev(1, 0, (16, 22)), solo[1]._fused.batch_dev(0, (16, 22)))
    with pytest.raises(ValueError):
        td3.Population(solo)                       # agents that already update on their own
