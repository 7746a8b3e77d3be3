"""The fused learners' replay path (td3_prep_kernel: cn_td3_update / cn_ddpg_update with batch == NULL) against the CPU statement
of tests/sampling_f64.py, read back through cn_td3_batch_dev / cn_ddpg_batch_dev: every sampled index exactly, at live sizes from 1
to 2^24 + 1 and on the degenerate *size_dev values, batches of 1, 129 and 4096 rows, seeds 0, 2^64 - 1 and a random one; the update
counter behind them (critic-only and actor updates, explicit batches in between, a captured graph replayed); TD3's target-policy
noise element by element within its float64 allowance, at the generator's extremes and with every wrong variant of the statement
breaking the allowance; the gathered batch being what the update's GEMMs consumed; and the Python agents' wiring of seed and live
size.  The networks are tiny (obs_dim 4, hidden 8): the GEMMs do not matter here.  `-s` prints the worst noise error / allowance
of every setting and the number of indices compared."""
import numpy as np
import pytest
import torch

import ddpg_f64 as D
import sampling_f64 as S
import td3_f64 as R
from learner_handle import LearnerHandle, alias, batch_struct, lib, mlp_struct, ring_fields

pytestmark = pytest.mark.gpu

OBS, HID = 4, 8
CFG = dict(gamma=0.99, tau=0.005, lr_actor=3e-4, lr_critic=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_v=0.22, max_w=2.0)
COUNT = dict(indices=0)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Handle(LearnerHandle):
    """One cn_td3 / cn_ddpg handle on its own copies of the parameters; `ring` (dict of device tensors, "size" an int64 [1]) or
    None for explicit batches only."""

    def __init__(self, algo, B, seed, ring=None, noise_std=0.2, noise_clip=0.5, P=None, pseed=0):
        self.algo, self.B, self.seed = algo, B, seed
        if P is None:
            g = torch.Generator().manual_seed(pseed)
            P = R.new_params(OBS, HID, g, dtype=torch.float32, device="cuda") if algo == "td3" else D.new_params(OBS, HID, g, device="cuda")
        self.P = {n: {k: v.detach().clone().contiguous() for k, v in p.items()} for n, p in P.items()}
        kw = dict(CFG, obs_dim=OBS, hidden=HID, batch=B, seed=seed, **{n: mlp_struct(self.P[n], R.NAMES) for n in self.P}, **ring_fields(ring))
        if algo == "td3":
            cfg = lib()[0].CnTd3Config(policy_delay=2, noise_std=noise_std, noise_clip=noise_clip, reserved=0.0, **kw)
        else:
            cfg = lib()[0].CnDdpgConfig(**kw)
        super().__init__(algo, cfg, (self.P, ring))

    def update(self, batch=None, do_actor=True, sync=True):
        super().update(*([int(do_actor)] if self.algo == "td3" else []), batch=batch_struct(batch), sync=sync)

    def ptr(self, what):
        return self._f("batch_dev")(self.h, what)

    def view(self, what):
        """A copy of the gathered buffer `what` (0: [s|a], 1: [s2|.], 2: r, 3: d, 4: noise)."""
        return self.batch_dev(what, {0: (self.B, OBS + 2), 1: (self.B, OBS + 2), 2: (self.B,), 3: (self.B,), 4: (self.B, 2)}[what])

    def loss(self):
        return super().loss((1,))


@pytest.fixture(scope="module")
def ring():
    """S.CAPACITY slots (2^24 + 4099: past every live size of the plan) whose rows encode the slot i: s = (i >> 12, i & 4095, ..),
    exact in float32 for every slot; a, r, s2, d carry encodings of their own.  ~0.8 GB."""
    i = torch.arange(S.CAPACITY, device="cuda", dtype=torch.int64)
    hi, lo = (i >> 12).float(), (i & 4095).float()
    rg = dict(s=torch.stack([hi, lo, lo + 0.5, -hi], 1).contiguous(), s2=torch.stack([lo, hi, -lo, hi + 0.25], 1).contiguous(),
              a=torch.stack([-hi, lo + 0.125], 1).contiguous(), r=(hi * 0.5 - lo).contiguous(), d=(i & 1).float().contiguous())
    del i, hi, lo
    torch.cuda.synchronize()
    yield rg
    rg.clear()
    torch.cuda.empty_cache()


def _check_indices(h, rg, k, size):
    """The rows update k gathered decode to S.indices(seed, k, B, size), and each equals, bit for bit, the ring row it names."""
    xs, x2, r, d = h.view(0), h.view(1), h.view(2), h.view(3)
    slot = (xs[:, 0].long() << 12) + xs[:, 1].long()
    want = torch.from_numpy(S.indices(h.seed, k, h.B, size)).cuda()
    bad = int((slot != want).sum())
    assert bad == 0, (h.algo, h.B, h.seed, k, size, bad, slot[:8].tolist(), want[:8].tolist())
    assert torch.equal(_bits(xs[:, :OBS]), _bits(rg["s"][want])), (h.algo, k, size)
    assert torch.equal(_bits(xs[:, OBS:]), _bits(rg["a"][want])), (h.algo, k, size)
    assert torch.equal(_bits(x2[:, :OBS]), _bits(rg["s2"][want])), (h.algo, k, size)
    assert torch.equal(_bits(r), _bits(rg["r"][want])), (h.algo, k, size)
    assert torch.equal(_bits(d), _bits(rg["d"][want])), (h.algo, k, size)
    COUNT["indices"] += h.B


def test_batch_view_arguments():
    _abi, L = lib()
    for f in (L.cn_td3_batch_dev, L.cn_ddpg_batch_dev):
        for what in (-1, 0, 4, 5):
            assert f(None, what) is None
    for algo in ("td3", "ddpg"):
        h = Handle(algo, 3, 1)
        try:
            for what in range(4):
                assert h.ptr(what)
            assert (h.ptr(4) is not None) == (algo == "td3")
            assert h.ptr(5) is None and h.ptr(-1) is None
        finally:
            h.close()


@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("algo", ("td3", "ddpg"))
def test_replay_indices_follow_the_statement_exactly(ring, algo, B):
    """Every update of S.index_plan(): the live sizes 1 ... 2^24 + 1 twice each, then *size_dev = 0, -1 and INT64_MIN (taken as
    1); TD3 alternates actor and critic-only updates."""
    before = COUNT["indices"]
    for seed in S.INDEX_SEEDS:
        rg = dict(ring, size=torch.zeros(1, dtype=torch.int64, device="cuda"))
        h = Handle(algo, B, seed, rg)
        try:
            for k, size in enumerate(S.index_plan()):
                rg["size"].fill_(size)
                h.update(None, do_actor=k % 2 == 1)
                _check_indices(h, rg, k, size)
        finally:
            h.close()
    print("\n%s B=%d: %d indices compared exactly (%d in the module so far)" % (algo, B, COUNT["indices"] - before, COUNT["indices"]))


def _explicit_batch(rg, B, seed, algo):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, 4096, (B,), generator=g).cuda()
    nz = (torch.randn((B, 2), generator=g) * 3).cuda() if algo == "td3" else None
    return rows, (rg["s"][rows].contiguous(), rg["a"][rows].contiguous(), rg["r"][rows].contiguous(), rg["s2"][rows].contiguous(),
                  rg["d"][rows].contiguous(), nz)


def _check_noise(h, k, std, clip):
    got = h.view(4).double().cpu().numpy()
    want, bound = S.target_noise(h.seed, k, h.B, std, clip)
    d = np.abs(got - want)
    ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
    return got, float(ratio.max())


@pytest.mark.parametrize("algo", ("td3", "ddpg"))
def test_counter_counts_every_update(ring, algo):
    """0 at create, +1 per update: replay and explicit-batch updates mixed, critic-only and actor updates; an explicit batch is
    gathered as passed (and its noise scaled and clipped like the drawn one)."""
    B, seed, size, std, clip = 129, 0x243F6A8885A308D3, 5003, 0.2, 0.5
    rg = dict(ring, size=torch.tensor([size], dtype=torch.int64, device="cuda"))
    h = Handle(algo, B, seed, rg, noise_std=std, noise_clip=clip)
    plan = [("replay", 0), ("replay", 1), ("explicit", 0), ("explicit", 1), ("replay", 0), ("explicit", 0), ("replay", 1),
            ("replay", 0), ("replay", 1)]
    try:
        for k, (kind, do_actor) in enumerate(plan):
            if kind == "replay":
                h.update(None, do_actor=do_actor)
                _check_indices(h, rg, k, size)
                if algo == "td3":
                    _, worst = _check_noise(h, k, std, clip)
                    assert worst <= 1.0, (k, worst)
            else:
                rows, batch = _explicit_batch(rg, B, k, algo)
                h.update(batch, do_actor=do_actor)
                xs = h.view(0)
                assert torch.equal(_bits(xs[:, :OBS]), _bits(batch[0])) and torch.equal(_bits(xs[:, OBS:]), _bits(batch[1]))
                assert torch.equal(_bits(h.view(1)[:, :OBS]), _bits(batch[3]))
                assert torch.equal(_bits(h.view(2)), _bits(batch[2])) and torch.equal(_bits(h.view(3)), _bits(batch[4]))
                if algo == "td3":
                    s32, c32 = torch.tensor(std, dtype=torch.float32), torch.tensor(clip, dtype=torch.float32)
                    want = torch.minimum(torch.maximum(batch[5] * s32.cuda(), -c32.cuda()), c32.cuda())
                    assert torch.equal(_bits(h.view(4)), _bits(want))
    finally:
        h.close()


@pytest.mark.parametrize("algo", ("td3", "ddpg"))
def test_captured_update_follows_the_counter(ring, algo):
    """One update captured into a hipGraph (one stream, a straight chain) and replayed five times: replay j gathers the indices of
    counter 2 + j, and an eager update after them those of counter 7 -- the counter lives on the device and the graph moves it."""
    B, seed, size = 129, 77, 65536
    rg = dict(ring, size=torch.tensor([size], dtype=torch.int64, device="cuda"))
    h = Handle(algo, B, seed, rg)
    try:
        for k in range(2):
            h.update(None, do_actor=True)
            _check_indices(h, rg, k, size)
        before = h.view(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            h.update(None, do_actor=True, sync=False)
        torch.cuda.synchronize()
        assert torch.equal(_bits(h.view(0)), _bits(before))            # capturing ran nothing
        for j in range(5):
            g.replay()
            torch.cuda.synchronize()
            _check_indices(h, rg, 2 + j, size)
        h.update(None, do_actor=False)
        _check_indices(h, rg, 7, size)
        del g
    finally:
        h.close()


@pytest.mark.parametrize("seed", S.NOISE_SEEDS)
def test_target_noise_matches_float64(ring, seed):
    """B = 4096 over 64 updates per setting: every element within its allowance (exactly zero where the statement is), and
    every wrong variant of the statement beyond the allowance somewhere."""
    rg = dict(ring, size=torch.tensor([1_000_000], dtype=torch.int64, device="cuda"))
    worst_variant = dict.fromkeys(S.NOISE_VARIANTS, 0.0)
    for std, clip in S.NOISE_SETTINGS:
        h = Handle("td3", S.NOISE_B, seed, rg, noise_std=std, noise_clip=clip)
        worst = 0.0
        try:
            for k in range(S.NOISE_UPDATES):
                h.update(None, do_actor=k % 2 == 0)
                got, w = _check_noise(h, k, std, clip)
                worst = max(worst, w)
                if std == 0 or clip == 0:
                    assert (got == 0).all(), (std, clip, k)
                want, bound = S.target_noise(seed, k, S.NOISE_B, std, clip)
                for v in S.NOISE_VARIANTS:
                    bad, _ = S.target_noise(seed, k, S.NOISE_B, std, clip, variant=v)
                    d = np.abs(got - bad)
                    r = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0))
                    worst_variant[v] = max(worst_variant[v], float(r.max()))
        finally:
            h.close()
        print("\nnoise seed %#x std %g clip %g: worst error / allowance %.3g over %d x %d x 2" % (
            seed, std, clip, worst, S.NOISE_UPDATES, S.NOISE_B))
        assert worst <= 1.0, (seed, std, clip, worst)
    print("wrong variants, worst error / allowance: " + ", ".join("%s %.3g" % kv for kv in worst_variant.items()))
    assert all(v > 1.0 for v in worst_variant.values()), worst_variant


@pytest.mark.parametrize("std,clip", ((1.0, 100.0), (0.2, 0.5)))
def test_target_noise_at_the_generators_extremes(ring, std, clip):
    """Searched seeds (S.find_extreme_seeds) put u1 = 2^-24 (r = 5.77), u1 = 1 (exactly zero), u2 = 0 (the sine column exactly
    zero), the quarter turns and u2 = 1 - 2^-24 on known (counter, row): there the device must be exact where the statement is
    zero and within the allowance elsewhere."""
    rg = dict(ring, size=torch.tensor([5003], dtype=torch.int64, device="cuda"))
    found = S.find_extreme_seeds(B=S.NOISE_B, counters=S.NOISE_UPDATES)
    for name, (seed, c, m) in sorted(found.items()):
        h = Handle("td3", S.NOISE_B, seed, rg, noise_std=std, noise_clip=clip)
        try:
            for k in range(c + 1):
                h.update(None, do_actor=k % 2 == 0)
            got, worst = _check_noise(h, c, std, clip)
            want, bound = S.target_noise(seed, c, S.NOISE_B, std, clip)
        finally:
            h.close()
        print("\n%-17s seed %d counter %d row %d: device (%.9g, %.9g)  float64 (%.9g, %.9g)  allowance (%.3g, %.3g)  batch worst %.3g" % (
            name, seed, c, m, got[m, 0], got[m, 1], want[m, 0], want[m, 1], bound[m, 0], bound[m, 1], worst))
        assert worst <= 1.0, (name, worst)
        for col in range(2):
            if want[m, col] == 0:
                assert got[m, col] == 0, (name, col, got[m, col])
        if name == "u1_one":
            assert (got[m] == 0).all()
        if name == "u2_zero":
            assert got[m, 1] == 0


def _small_ring(cap, size, seed):
    g = torch.Generator().manual_seed(seed)
    rg = dict(s=torch.randn((cap, OBS), generator=g) * 0.5, a=torch.stack([torch.rand(cap, generator=g) * 0.22,
                                                                            torch.rand(cap, generator=g) * 4 - 2], 1),
              r=2 + 0.5 * torch.randn(cap, generator=g), s2=torch.randn((cap, OBS), generator=g) * 0.5,
              d=(torch.rand(cap, generator=g) < 0.3).float())
    rg = {k: v.float().cuda().contiguous() for k, v in rg.items()}
    rg["size"] = torch.tensor([size], dtype=torch.int64, device="cuda")
    return rg


@pytest.mark.parametrize("algo", ("td3", "ddpg"))
def test_view_is_what_the_update_consumed(algo):
    """A replay-path handle equals, weights and loss bit for bit over four updates (actor steps included), a second handle fed
    the first one's gathered rows -- and for TD3 its read-back noise as explicit target_noise: with noise_std 1 and noise_clip 8
    nothing clips (|z| <= 5.77) and z x 1 is exact, so the explicit path rebuilds the same noise.  Live size 5003."""
    B, size = 129, 5003
    rg = _small_ring(8192, size, 11)
    a = Handle(algo, B, 0x9E3779B97F4A7C15, rg, noise_std=1.0, noise_clip=8.0, pseed=5)
    b = Handle(algo, B, 0, None, noise_std=1.0, noise_clip=8.0, pseed=5)
    P0 = {n: {key: v.clone() for key, v in p.items()} for n, p in a.P.items()}
    try:
        assert all(torch.equal(a.P[n][key], b.P[n][key]) for n in a.P for key in R.NAMES)
        for k in range(4):
            a.update(None, do_actor=k % 2 == 0)
            xs, x2 = a.view(0), a.view(1)
            nz = a.view(4) if algo == "td3" else None
            if nz is not None:
                assert float(nz.abs().max()) <= S.r_max()
            batch = (xs[:, :OBS].contiguous(), xs[:, OBS:].contiguous(), a.view(2), x2[:, :OBS].contiguous(), a.view(3), nz)
            b.update(batch, do_actor=k % 2 == 0)
            if nz is not None:
                assert torch.equal(_bits(b.view(4)), _bits(nz))
            for n in a.P:
                for key in R.NAMES:
                    assert torch.equal(_bits(a.P[n][key]), _bits(b.P[n][key])), (algo, k, n, key)
            assert torch.equal(_bits(a.loss()), _bits(b.loss())), (algo, k)
        assert not all(torch.equal(a.P[n][key], P0[n][key]) for n in a.P for key in R.NAMES)     # the updates did step them
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("algo", ("td3", "ddpg"))
def test_agent_replay_indices_follow_the_statement(algo):
    """crowdnav's Agent with the fused update, filled through DeviceReplay.add_masked (cn_replay_write) past the point where its
    ring wraps, learn() between the writes: update k samples S.indices(agent._noise_seed, k, B, live size at that moment), and
    every sampled slot holds the transition the host expects there.  Catches a replay_size_dev bound to the wrong scalar and a
    seed other than the documented one."""
    _abi, L = lib()
    if algo == "td3":
        from crowdnav.td3 import Agent
    else:
        from crowdnav.ddpg import Agent
    B, cap = 16, 50
    agent = Agent(obs_dim=OBS, hidden=HID, batch_size=B, memory_size=cap, device="cuda", seed=5)
    agent.enable_fused_update()
    hnd = agent._fused.h
    view = L.cn_td3_batch_dev if algo == "td3" else L.cn_ddpg_batch_dev
    rng = np.random.default_rng(3)
    slot_t = np.full(cap, -1, dtype=np.int64)
    t = live = k = 0
    for launch in range(48):
        n = 10
        keep = rng.random(n) < 0.7
        ids = np.full(n, (1 << 23) + launch, dtype=np.int64)        # rows not kept: an id no slot holds
        for i in np.flatnonzero(keep):
            ids[i] = t
            slot_t[t % cap] = t
            t += 1
        idt = torch.from_numpy(ids).cuda()
        hi, lo = (idt >> 12).float(), (idt & 4095).float()
        s = torch.stack([hi, lo, lo * 0.5, -hi], 1)
        agent.memory.add_masked(s, torch.zeros((n, 2), device="cuda"), torch.zeros(n, device="cuda"), s * 0.25,
                                torch.zeros(n, dtype=torch.bool, device="cuda"), torch.from_numpy(keep).cuda())
        live = min(cap, live + int(keep.sum()))
        loss = agent.learn(launch)
        assert (loss is not None) == (live > B), (launch, live)
        if loss is None:
            continue
        torch.cuda.synchronize()
        xs = alias(view(hnd, 0), (B, OBS + 2)).clone()
        got_t = ((xs[:, 0].long() << 12) + xs[:, 1].long()).cpu().numpy()
        want = S.indices(agent._noise_seed, k, B, live)
        assert np.array_equal(got_t % cap, want), (algo, launch, k, live)
        assert np.array_equal(got_t, slot_t[want]), (algo, launch, k)
        k += 1
    assert t > 2 * cap and k >= 30, (t, k)
    del agent
