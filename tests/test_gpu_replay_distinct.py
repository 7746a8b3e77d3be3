"""Replay sampling without replacement (CN_SAMPLE_DISTINCT, include/crowdnav.h next to cn_td3_batch_dev) against the CPU statement of
tests/replay_distinct_ref.py, every comparison an equality of integers: cn_replay_sample_indices over the statement's whole plan in
both modes; the four fused learners on rings whose rows encode their slot, read back through cn_*_batch_dev; batches larger than the
ring; a live size rewritten on the device; the default mode and the setters' refusals; a captured update; and the Python wiring
(DeviceReplay.sample(replace=False), the agents' replay_sample).  The networks are tiny (obs_dim 5, hidden 16): the GEMMs do not
matter here."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_distinct_ref as S
import sampling_f64
from learner_handle import LearnerHandle, err, lib, ring_fields, stream

pytestmark = pytest.mark.gpu

OBS, HID = 5, 16
FAMILIES = ("td3", "ddpg", "dqn", "sac")
CAP = 8192                                      # the learners' ring: past every live size they are given


# ---- cn_replay_sample_indices ---------------------------------------------------------------------------------------------------
def _sample_indices(seed, counter, B, size_dev, mode, out):
    _abi, L = lib()
    rc = L.cn_replay_sample_indices(seed, counter, B, C.c_void_p(size_dev.data_ptr()), mode, C.c_void_p(out.data_ptr()), 0, stream())
    assert rc == 0, err()


@pytest.fixture(scope="module")
def seam():
    """Both modes over the statement's plan: {(mode, size, B, seed, counter): rows}, the launches of one size read back together."""
    size_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    combos = [(mode, B, seed, c) for mode in (1, 0) for B in S.BATCHES for seed in S.SEEDS for c in S.COUNTERS]
    out = torch.full((len(combos), max(S.BATCHES) + 1), -7, dtype=torch.int64, device="cuda")
    got = {}
    for size in S.LIVE_SIZES + S.DEGENERATE_SIZES:
        size_dev.fill_(size)
        out.fill_(-7)
        for j, (mode, B, seed, c) in enumerate(combos):
            _sample_indices(seed, c, B, size_dev, mode, out[j])
        host = out.cpu().numpy()
        for j, (mode, B, seed, c) in enumerate(combos):
            assert (host[j, B:] == -7).all(), (size, mode, B)             # nothing past the B rows asked for
            got[(mode, size, B, seed, c)] = host[j, :B].copy()
    return got


def test_sample_indices_mode_1_equals_the_statement(seam):
    n = 0
    for (mode, size, B, seed, c), rows in seam.items():
        if mode != 1:
            continue
        want = S.rows(seed, c, B, size)
        assert np.array_equal(rows, want), (size, B, seed, c, rows[:8], want[:8])
        if B <= S.live(size):
            assert len(set(rows.tolist())) == B, (size, B)
        n += B
    print("\n%d indices of mode 1 compared exactly" % n)
    assert n == (len(S.LIVE_SIZES) + len(S.DEGENERATE_SIZES)) * sum(S.BATCHES) * len(S.SEEDS) * len(S.COUNTERS)


def test_sample_indices_mode_0_equals_the_draw_with_replacement(seam):
    n = 0
    for (mode, size, B, seed, c), rows in seam.items():
        if mode != 0:
            continue
        assert np.array_equal(rows, sampling_f64.indices(seed, c, B, size)), (size, B, seed, c)
        n += B
    assert n > 0


def test_sample_indices_refusals():
    _abi, L = lib()
    size_dev = torch.ones(1, dtype=torch.int64, device="cuda")
    out = torch.zeros(4, dtype=torch.int64, device="cuda")
    sp, op = C.c_void_p(size_dev.data_ptr()), C.c_void_p(out.data_ptr())
    for args, text in (((1, 0, 4, None, 1, op), "null"), ((1, 0, 4, sp, 1, None), "null"), ((1, 0, 0, sp, 1, op), "B < 1"),
                       ((1, 0, 4, sp, 2, op), "mode"), ((1, 0, 4, sp, -1, op), "mode")):
        assert L.cn_replay_sample_indices(*args, 0, stream()) == -1 and text in err(), (args, err())
    torch.cuda.synchronize()
    assert not out.any()


# ---- the four learners ----------------------------------------------------------------------------------------------------------
def _mlp(g, n_in, H, n_out):
    """(struct, tensors): Linear(n_in, H) - Linear(H, H) - Linear(H, n_out), small weights."""
    _abi, _ = lib()
    shapes = ((H, n_in), (H,), (H, H), (H,), (n_out, H), (n_out,))
    ts = [(torch.randn(s, generator=g) * 0.1).cuda().contiguous() for s in shapes]
    return _abi.CnTd3Mlp(*[t.data_ptr() for t in ts]), ts


def _ring(n):
    """CAP slots whose rows encode the slot i (exact in float32): s[:, 0] = i, s2[:, 0] = i + 0.25, a = (i mod 3, i + 0.125),
    r = 0.5 i - 3, d = 1 where 7 i mod 5 == 0; live size n (int64 on the device)."""
    i = torch.arange(CAP, device="cuda", dtype=torch.int64)
    f = i.float()
    lo = (i & 63).float() / 64
    return dict(s=torch.stack([f, lo, lo - 0.5, -lo, lo * 0.25], 1).contiguous(),
                s2=torch.stack([f + 0.25, -lo, lo, lo + 0.5, lo * 0.125], 1).contiguous(),
                a=torch.stack([(i % 3).float(), f + 0.125], 1).contiguous(), r=(f * 0.5 - 3).contiguous(),
                d=((7 * i) % 5 == 0).float().contiguous(), size=torch.tensor([n], dtype=torch.int64, device="cuda"))


class Handle(LearnerHandle):
    """One learner handle of `family` on its own tiny networks, sampling the ring `rg`."""

    def __init__(self, family, B, seed, rg):
        _abi, _ = lib()
        self.B, self.seed, self.rg = B, seed, rg
        g = torch.Generator().manual_seed(1)
        keep = [rg]

        def mlp(n_in, n_out, H=HID):
            st, ts = _mlp(g, n_in, H, n_out)
            keep.append(ts)
            return st
        rp = dict(ring_fields(rg), seed=seed)
        adam = dict(gamma=0.99, beta1=0.9, beta2=0.999, eps=1e-8, max_v=0.22, max_w=2.0)
        if family == "td3":
            cfg = _abi.CnTd3Config(obs_dim=OBS, hidden=HID, batch=B, policy_delay=2, tau=0.005, lr_actor=3e-4, lr_critic=3e-4, noise_std=0.2,
                                   noise_clip=0.5, reserved=0.0, actor=mlp(OBS, 2), actor_t=mlp(OBS, 2), q1=mlp(OBS + 2, 1),
                                   q1_t=mlp(OBS + 2, 1), q2=mlp(OBS + 2, 1), q2_t=mlp(OBS + 2, 1), **adam, **rp)
        elif family == "ddpg":
            cfg = _abi.CnDdpgConfig(obs_dim=OBS, hidden=HID, batch=B, tau=0.001, lr_actor=1e-4, lr_critic=1e-3, actor=mlp(OBS, 2),
                                    actor_t=mlp(OBS, 2), critic=mlp(OBS + 2, 1), critic_t=mlp(OBS + 2, 1), **adam, **rp)
        elif family == "dqn":
            cfg = _abi.CnDqnConfig(obs_dim=OBS, obs_ld=OBS, hidden=HID, batch=B, gamma=0.99, lr=2.5e-4, rho=0.9, eps=1e-6, target_every=10000,
                                   learn_start=0, q=mlp(OBS, 3), q_t=mlp(OBS, 3), **rp)
        else:
            st, ts = _mlp(g, OBS, HID, 2)
            extra = [(torch.randn(s, generator=g) * 0.1).cuda().contiguous() for s in ((2, HID), (2,))]
            keep += [ts, extra]
            actor = _abi.CnSacActor(*[t.data_ptr() for t in ts + extra])
            cfg = _abi.CnSacConfig(obs_dim=OBS, hidden=HID, hidden_v=2, batch=B, gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_v=3e-4, lr_q=3e-4,
                                   beta1=0.9, beta2=0.999, eps=1e-8, max_v=0.22, max_w=2.0, log_std_min=-20.0, log_std_max=2.0,
                                   mean_lambda=1e-3, std_lambda=1e-3, z_lambda=0.0, logp_eps=1e-6, soft_update=0, reserved=0, actor=actor,
                                   q=mlp(OBS + 2, 1), v=mlp(OBS, 1, 2), v_t=mlp(OBS, 1, 2), **rp)
        super().__init__(family, cfg, keep)

    def update(self, k=0, sync=True):
        super().update(*([int(k % 2 == 1)] if self.family == "td3" else []), sync=sync)

    def gathered(self):
        """(slots int64 [B], dict of what the update gathered for its B rows) of the last update."""
        B = self.B
        if self.family == "dqn":
            x = self.batch_dev(0, (2 * B, OBS))
            got = dict(s=x[:B], s2=x[B:], r=self.batch_dev(1, (B,)), d=self.batch_dev(2, (B,)), a0=self.batch_dev(3, (B,), "<i4").float())
        else:
            xs, x2 = self.batch_dev(0, (B, OBS + 2)), self.batch_dev(1, (B, OBS + 2))
            got = dict(s=xs[:, :OBS], s2=x2[:, :OBS], r=self.batch_dev(2, (B,)), d=self.batch_dev(3, (B,)), a=xs[:, OBS:])
        return got["s"][:, 0].long(), got

    def check(self, want):
        """The last update gathered exactly the ring rows `want` (numpy int64 [B]): every column of every row, bit for bit."""
        slot, got = self.gathered()
        w = torch.from_numpy(np.asarray(want, dtype=np.int64)).cuda()
        assert torch.equal(slot, w), (self.family, self.B, slot[:8].tolist(), w[:8].tolist())
        rg = self.rg
        for key in ("s", "s2", "r", "d"):
            assert torch.equal(got[key], rg[key][w]), (self.family, key)
        if "a" in got:
            assert torch.equal(got["a"], rg["a"][w]), self.family
        else:
            assert torch.equal(got["a0"], rg["a"][w][:, 0]), self.family


def _check_dqn_plan(h, want):
    """flags[2] = F, the number of final rows among the sample; chunk marks exactly B + F stacked rows: the B s rows and the s2 row
    of every final sample, B of them in chunk 1 and F in chunk 2."""
    B = h.B
    final = (h.rg["d"][torch.from_numpy(want).cuda()] != 0).cpu().numpy()
    F = int(final.sum())
    flags = h.batch_dev(5, (8,), "<i4").cpu().numpy()
    chunk = h.batch_dev(4, (2 * B,), "<i4").cpu().numpy()
    assert flags[0] == 1 and flags[2] == F and flags[1] == (1 if F else 0), (flags.tolist(), F)
    assert (chunk[:B] != 0).all() and np.array_equal(chunk[B:] != 0, final), (chunk.tolist(), final.tolist())
    assert int((chunk != 0).sum()) == B + F and int((chunk == 1).sum()) == B and int((chunk == 2).sum()) == F


@pytest.mark.parametrize("n,B", ((64, 64), (65, 64), (5003, 128), (37, 128)))
@pytest.mark.parametrize("family", FAMILIES)
def test_learners_gather_the_statements_rows(family, n, B):
    """Mode 1, three consecutive updates of one handle: the rows are S.rows for counters 0, 1, 2.  n = B = 64: a permutation of the
    ring (with replacement, 64 draws from 64 are all distinct with probability 64! / 64^64 ~ 1e-27).  n = 65, B = 64: DQN's first
    live update.  B = 128 > n = 37: every ring row comes up 3 or 4 times."""
    rg = _ring(n)
    seed = 0x243F6A8885A308D3
    h = Handle(family, B, seed, rg)
    try:
        assert h.set_replay_sample(1) == 0, err()
        for k in range(3):
            h.update(k)
            want = S.rows(seed, k, B, n)
            h.check(want)
            slot = h.gathered()[0].cpu().numpy()
            if B <= n:
                assert len(set(slot.tolist())) == B
            if B == n:
                assert np.array_equal(np.sort(slot), np.arange(n))
            if B > n:
                assert set(np.bincount(slot, minlength=n).tolist()) <= {B // n, -(-B // n)}
            if family == "dqn":
                _check_dqn_plan(h, want)
                assert int(h.batch_dev(8, (2,), "<i4").cpu().numpy().view(np.uint64)[0]) == k + 1
    finally:
        h.close()


def test_live_size_rewritten_on_the_device_between_updates():
    seed, B = 77, 128
    rg = _ring(37)
    h = Handle("td3", B, seed, rg)
    try:
        assert h.set_replay_sample(1) == 0
        h.update(0)
        h.check(S.rows(seed, 0, B, 37))
        rg["size"].fill_(5003)                      # a device-side write, as cn_replay_write's
        h.update(1)
        want = S.rows(seed, 1, B, 5003)
        h.check(want)
        slot = h.gathered()[0]
        assert int(slot.max()) < 5003 and int(slot.max()) >= 37 and len(set(slot.tolist())) == B
    finally:
        h.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_default_mode_is_the_draw_with_replacement_and_bad_modes_are_refused(family):
    seed, B, n = 5, 64, 64
    rg = _ring(n)
    fresh, zero = Handle(family, B, seed, rg), Handle(family, B, seed, rg)
    try:
        assert zero.set_replay_sample(0) == 0
        for h in (fresh, zero):
            for k in range(2):
                h.update(k)
                h.check(sampling_f64.indices(seed, k, B, n))
        h = fresh
        for before in (0, 1):                       # a refused mode leaves the handle's mode alone, whichever it is
            assert h.set_replay_sample(before) == 0
            for bad in (2, -1):
                assert h.set_replay_sample(bad) == -1 and "cn_%s_set_replay_sample" % family in err() and "mode" in err(), err()
        k = 2
        h.update(k)                                 # still mode 1
        h.check(S.rows(seed, k, B, n))
        assert getattr(h.L, "cn_%s_set_replay_sample" % family)(None, 1) == -1 and "null handle" in err()
    finally:
        fresh.close(); zero.close()


def test_captured_update_keeps_its_mode_and_follows_the_counter():
    """One TD3 update in mode 1 captured into a graph on one stream and replayed three times: the rows of counters c, c + 1, c + 2.
    The setter called after the capture changes the next enqueued update, not the captured one."""
    seed, B, n = 0x9E3779B97F4A7C15, 64, 65
    rg = _ring(n)
    h = Handle("td3", B, seed, rg)
    try:
        assert h.set_replay_sample(1) == 0
        for k in range(2):
            h.update(k)
            h.check(S.rows(seed, k, B, n))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            h.update(0, sync=False)
        torch.cuda.synchronize()
        h.check(S.rows(seed, 1, B, n))                                  # capturing ran nothing
        assert h.set_replay_sample(0) == 0
        for j in range(3):
            g.replay()
            torch.cuda.synchronize()
            h.check(S.rows(seed, 2 + j, B, n))
        h.update(1)
        h.check(sampling_f64.indices(seed, 5, B, n))
        del g
    finally:
        h.close()


# ---- the Python wiring ------------------------------------------------------------------------------------------------------------
def _fill(mem, n, D):
    i = torch.arange(n, device="cuda")
    s = torch.zeros((n, D), device="cuda")
    s[:, 0] = i.float()
    mem.add(s, torch.zeros((n, 2), device="cuda"), i.float() * 0.5, s + 0.25, (i % 4 == 0))


def test_device_replay_sample_without_replacement():
    from crowdnav.td3 import DeviceReplay
    for cap in (64, 100):
        mem = DeviceReplay(cap, OBS, "cuda")
        _fill(mem, 64, OBS)
        for call in range(2):
            s, a, r, s2, d = mem.sample(64, replace=False)
            slot = s[:, 0].long().cpu().numpy()
            assert np.array_equal(np.sort(slot), np.arange(64)), (cap, call)
            assert np.array_equal(slot, S.rows(mem.sample_seed, call, 64, 64)), (cap, call)
            assert torch.equal(r[:, 0], s[:, 0] * 0.5) and torch.equal(s2[:, 0], s[:, 0] + 0.25) and torch.equal(d[:, 0], (s[:, 0].long() % 4 == 0).float())
        s = mem.sample(16, replace=False)[0]
        assert len(set(s[:, 0].tolist())) == 16 and mem.sample_calls == 3
        assert mem.sample(16)[0].shape == (16, OBS)                      # the default path, untouched
    with pytest.raises(RuntimeError):
        DeviceReplay(8, OBS, "cpu").sample(4, replace=False)


@pytest.mark.parametrize("family", FAMILIES)
def test_agents_pass_replay_sample_to_their_fused_update(family):
    """Agent(replay_sample="without"): the fused update's rows are S.rows(the handle's seed, k, B, len(memory)); the default agent's
    are sampling_f64.indices; anything else is a ValueError."""
    import importlib
    mod = importlib.import_module("crowdnav." + family)
    B, n = 16, 17
    kw = dict(obs_dim=OBS, batch_size=B, memory_size=40, device="cuda", seed=3)
    kw.update(dict(hidden=(HID, HID), learn_start=B) if family == "dqn" else dict(hidden=HID))
    with pytest.raises(ValueError):
        mod.Agent(replay_sample="distinct", **kw)
    for name, ref in (("without", S.rows), ("with", sampling_f64.indices)):
        agent = mod.Agent(replay_sample=name, **kw) if name == "without" else mod.Agent(**kw)
        agent.enable_fused_update()
        assert agent._fused.replay_sample == name
        _fill(agent.memory, n, OBS)
        for k in range(2):
            assert agent.learn(k) is not None
            torch.cuda.synchronize()
            x = agent._fused.batch_dev(0, (2 * B, OBS) if family == "dqn" else (B, OBS + 2))
            slot = x[:B, 0].long().cpu().numpy()
            assert np.array_equal(slot, ref(agent._fused.cfg.seed, k, B, n)), (family, name, k)
            assert (len(set(slot.tolist())) == B) or name == "with"
        del agent
