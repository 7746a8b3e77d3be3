"""The fused TD3 actor (actor_tile: cn_actor_forward and cn_rollout_policy's policy phase) and the output stage cn_policy_tail
against the float64 statement of tests/actor_f64.py, element by element within its bound: every observation width around the
kernel's staging chunks (512 columns), its 64 KB LDS edge (Dp 736 / 768), the simulator's widths and the kernel's limit; ragged
batches up to rows above 2^16; the exploration noise under several (seed, counter) keys, a counter above 2^32 and a seed with its
high bits set; and cn_rollout_policy's actions on the observations the kernel itself read, without cn_actor_forward in the loop.
linear3 is scaled so the logits span about +-4 (the heads stay out of saturation, where an error in the logits would vanish) and
sigma = 0.1 (the noise is rarely clipped away).  Each wrong variant of the reference must break the bound somewhere.
The forward bound is the strict worst case (tests/actor_f64.py): on random observations the kernel's error sits 3 to 5 orders of
magnitude below it, so one input column among a thousand can go missing unseen.  Every width therefore also runs with its edge
columns (edge_columns: both sides of each 512-column staging chunk boundary, the last 32-input block, the first and last column)
scaled by EDGE_SCALE, and shows that it sees each of them: the reference with any one of them zeroed breaks the bound.
`-s` prints the worst error / bound of every case."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import actor_f64 as A
from learner_handle import lib, stream
from td3_f64 import worst_ratio

pytestmark = pytest.mark.gpu

MAX_V, MAX_W = float(np.float32(0.22)), float(np.float32(2.0))     # the kernels take float32 arguments
SIGMA = float(np.float32(0.1))
KEYS = ((0, 1), (0xD1B54A32D192ED03, 7), (12345, (1 << 32) + 5), ((1 << 63) | 0x5DEECE66D, (1 << 40) + 3))
WIDTHS = (1, 31, 32, 33,            # the narrow limit and one 32-input block
          363, 370, 398,            # the original, real-world and risk layouts at 360 rays
          512, 513,                 # the first 512-column staging chunk, and a second chunk from Dp 544
          736, 737,                 # Dp 736 is the widest tile in 64 KB of LDS; Dp 768 takes hipFuncSetAttribute's path
          758, 790,                 # 720 rays with K = 8 (BASELINE configs[4]) and K = 16
          1024, 1025,               # the second chunk full; a third from Dp 1056
          1095,                     # 1025 rays, K = 16: the simulator's widest observation
          2272)                     # the kernel's limit (160 KiB of LDS)
CN_ERR_CONFIG = -2
EDGE_SCALE = 256.0          # edge columns' observations x 256: one such column's share of the logits is far above the bound
# the widest world cn_rollout_policy accepts: 1025 rays with K = 16 (obs_dim 1095) does not fit 8 environments in one CU's LDS
# (0, 4, 20, 60, 100 and 128 pedestrians tried); with K = 16 and no pedestrians 965 rays do and 966 do not: obs_dim 1035, Dp 1056,
# three staging chunks
WIDEST_WORLD = dict(n_rays=965, k_obstacles=16, n_peds=0, room_half=3.0)


def make_actor(D, seed, obs):
    """nn.Linear's initialisation as float32 values (float64 tensors on the device), linear3 rescaled per output so that the
    logits on `obs` span +-4."""
    g = torch.Generator().manual_seed(seed)

    def lin(i, o):
        k = 1.0 / math.sqrt(i)
        return [((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) * k).float().double().cuda() for s in ((o, i), (o,))]
    p = dict(zip(("w1", "b1", "w2", "b2", "w3", "b3"), lin(D, 256) + lin(256, 256) + lin(256, 2)))
    lg, _ = A.logits_and_bound(p, obs.double())
    c = 4.0 / lg.abs().amax(0).clamp_min(1e-30)
    p["w3"] = (p["w3"] * c[:, None]).float().double()
    p["b3"] = (p["b3"] * c).float().double()
    return p


class Packed:
    """p in cn_actor_pack_weights' layout (as crowdnav.td3.FusedActorMixin.sync_fused_weights lays it out)."""

    def __init__(self, p):
        _abi, L = lib()
        D = p["w1"].shape[1]
        Dp = (D + 31) // 32 * 32
        w1t = torch.zeros((Dp, 256), dtype=torch.float32, device="cuda")
        w1t[:D] = p["w1"].T.float()
        w2t = p["w2"].T.float().contiguous()
        self.w1p, self.w2p = torch.empty_like(w1t), torch.empty_like(w2t)
        _abi.check(L.cn_actor_pack_weights(C.c_void_p(w1t.data_ptr()), Dp, C.c_void_p(self.w1p.data_ptr()), 0, stream()))
        _abi.check(L.cn_actor_pack_weights(C.c_void_p(w2t.data_ptr()), 256, C.c_void_p(self.w2p.data_ptr()), 0, stream()))
        self.f = {k: p[k].float().contiguous() for k in ("b1", "b2", "w3", "b3")}
        self.w = _abi.CnActorWeights(w1p=self.w1p.data_ptr(), b1=self.f["b1"].data_ptr(), w2p=self.w2p.data_ptr(),
                                     b2=self.f["b2"].data_ptr(), w3=self.f["w3"].data_ptr(), b3=self.f["b3"].data_ptr(),
                                     obs_dim=D, obs_dim_padded=Dp, hidden=256, reserved=0)
        torch.cuda.synchronize()

    def forward(self, obs, sigma=0.0, seed=0, counter=0, max_v=MAX_V, max_w=MAX_W):
        _abi, L = lib()
        out = torch.full((obs.shape[0], 2), float("nan"), device="cuda")
        _abi.check(L.cn_actor_forward(C.byref(self.w), C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), obs.shape[0],
                                      max_v, max_w, sigma, seed, counter, 0, stream()))
        torch.cuda.synchronize()
        return out


def edge_columns(D):
    """The input columns at the kernel's edges for width D: the first and the last, the first of the last 32-input block (the
    zero-padded rows of the packed linear1 follow it), and both sides of every 512-column staging chunk boundary."""
    Dp = (D + 31) // 32 * 32
    cols = {0, Dp - 32, D - 1}
    for c0 in range(512, D, 512):
        cols |= {c0 - 1, c0}
    return sorted(cols)


def _case(D, n, seed, edge_scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    obs = torch.randn((n, D), generator=g)
    obs[:, edge_columns(D)] *= edge_scale
    obs = obs.cuda()
    p = make_actor(D, seed, obs)
    return obs, p, Packed(p)


def _check(got, want, bound, what):
    r = worst_ratio(got, want, bound)
    assert torch.isfinite(got).all(), what
    assert r <= 1.0, (what, r)
    return r


@pytest.mark.parametrize("D", WIDTHS)
def test_actor_forward_widths(D):
    """cn_actor_forward at every width of WIDTHS (a ragged batch of 100 rows: six full tiles and four rows), noise off and on."""
    obs, p, pk = _case(D, 100, D)
    want, bound = A.act(p, obs.double(), MAX_V, MAX_W)
    r_fwd = _check(pk.forward(obs), want, bound, (D, "forward"))
    r_noise = 0.0
    for seed, counter in KEYS[1:3]:
        want, bound = A.act(p, obs.double(), MAX_V, MAX_W, SIGMA, seed, counter)
        r_noise = max(r_noise, _check(pk.forward(obs, SIGMA, seed, counter), want, bound, (D, "noise", seed, counter)))
    # the noise alone at this width: linear3 zeroed and b3 = (-100, 0) make the logits exactly (-100, 0), so v's head is 0 and
    # w's is tanh(0) = 0, and the bound is the noise allowance by itself rather than the forward bound
    q = dict(p, w3=torch.zeros_like(p["w3"]), b3=torch.tensor([-100.0, 0.0], dtype=torch.float64, device="cuda"))
    qk = Packed(q)
    r_alone = 0.0
    for seed, counter in KEYS[1:3]:
        want, bound = A.act(q, obs.double(), MAX_V, MAX_W, SIGMA, seed, counter)
        r_alone = max(r_alone, _check(qk.forward(obs, SIGMA, seed, counter), want, bound, (D, "noise alone", seed, counter)))
    print("cn_actor_forward D %4d: forward %.3g, noise %.3g, noise alone %.3g of the bound" % (D, r_fwd, r_noise, r_alone))


@pytest.mark.parametrize("D", WIDTHS)
def test_actor_forward_sees_its_edges(D):
    """The width's edge columns scaled by EDGE_SCALE: the kernel stays within the bound, and the reference with any single edge
    column zeroed does not -- a kernel that dropped, shifted or misplaced the column at a chunk boundary or in the last block
    would fail this width."""
    obs, p, pk = _case(D, 100, D, EDGE_SCALE)
    got = pk.forward(obs)
    want, bound = A.act(p, obs.double(), MAX_V, MAX_W)
    r = _check(got, want, bound, (D, "edges"))
    seen = {}
    for c in edge_columns(D):
        o = obs.double().clone()
        o[:, c] = 0
        seen[c] = worst_ratio(got, *A.act(p, o, MAX_V, MAX_W))
        assert seen[c] > 1.0, (D, c, seen[c])
    print("cn_actor_forward D %4d, edges x %g: %.3g of the bound; any edge column zeroed: >= %.3g x the bound %s"
          % (D, EDGE_SCALE, r, min(seen.values()), sorted(seen)))


@pytest.mark.parametrize("n", (1, 15, 16, 17, 65541))
def test_actor_forward_batches(n):
    """Batch sizes around the 16-row tile and one large ragged batch whose rows pass 2^16 (a tile-local or 16-bit noise key would
    show), under every key of KEYS."""
    obs, p, pk = _case(398, n, n)
    want, bound = A.act(p, obs.double(), MAX_V, MAX_W)
    r_fwd = _check(pk.forward(obs), want, bound, (n, "forward"))
    r_noise = 0.0
    for seed, counter in (KEYS if n < 1000 else KEYS[2:]):
        want, bound = A.act(p, obs.double(), MAX_V, MAX_W, SIGMA, seed, counter)
        r_noise = max(r_noise, _check(pk.forward(obs, SIGMA, seed, counter), want, bound, (n, "noise", seed, counter)))
    print("cn_actor_forward n %5d: forward %.3g, noise %.3g of the bound" % (n, r_fwd, r_noise))


def test_actor_forward_refuses_past_its_lds_tile():
    """obs_dim 2273 (Dp 2304) needs more than 160 KiB of LDS: CN_ERR_CONFIG, before anything is launched."""
    _abi, L = lib()
    z = torch.zeros(16, device="cuda")
    for D, rc in ((2273, CN_ERR_CONFIG), (4000, CN_ERR_CONFIG)):
        w = _abi.CnActorWeights(w1p=z.data_ptr(), b1=z.data_ptr(), w2p=z.data_ptr(), b2=z.data_ptr(), w3=z.data_ptr(),
                                b3=z.data_ptr(), obs_dim=D, obs_dim_padded=(D + 31) // 32 * 32, hidden=256, reserved=0)
        assert L.cn_actor_forward(C.byref(w), C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr()), 1, MAX_V, MAX_W, 0.0, 0, 0, 0,
                                  None) == rc
        assert b"too wide" in L.cn_last_error()


def _tail(lg, max_v, max_w, sigma, seed, counter):
    _abi, L = lib()
    out = torch.full_like(lg, float("nan"))
    _abi.check(L.cn_policy_tail(C.c_void_p(lg.data_ptr()), C.c_void_p(out.data_ptr()), lg.shape[0], max_v, max_w, sigma, seed,
                                counter, 0, stream()))
    torch.cuda.synchronize()
    return out


def test_policy_tail_heads_noise_and_clip():
    """cn_policy_tail: logits over +-4, the tanh branch point 0.625, and the extremes +-20, +-100, +-inf; noise off and under
    every key; then the noise alone (v's head at 0 by l0 = -inf, w's at tanh(0) = 0, no clip within reach) on 2^20 rows.
    Where the float64 value lies beyond a clip bound by more than the bound, the kernel returns that bound exactly."""
    g = torch.Generator().manual_seed(5)
    ext = torch.tensor([0.0, -0.0, 0.625, -0.625, 20.0, -20.0, 100.0, -100.0, math.inf, -math.inf])
    col = torch.cat([torch.rand(4086, generator=g) * 8 - 4, ext])
    lg = torch.stack([col, col.flip(0)], 1).float().cuda().contiguous()
    n = lg.shape[0]
    hi = torch.tensor([MAX_V, MAX_W], dtype=torch.float64, device="cuda")
    lo = torch.tensor([0.0, -MAX_W], dtype=torch.float64, device="cuda")
    worst = {}
    for sigma, keys in ((0.0, KEYS[:1]), (SIGMA, KEYS), (1.0, KEYS[1:2])):
        for seed, counter in keys:
            got = _tail(lg, MAX_V, MAX_W, sigma, seed, counter)
            want, bound = A.act(None, lg.double(), MAX_V, MAX_W, sigma, seed, counter)
            worst[sigma] = max(worst.get(sigma, 0.0), _check(got, want, bound, ("tail", sigma, seed, counter)))
            assert bool((got[:, 0] >= 0).all() and (got[:, 0] <= MAX_V).all() and (got[:, 1].abs() <= MAX_W).all())
            # the unclipped float64 value: beyond a bound by more than the allowance -> exactly that bound
            raw, _ = A.act(None, lg.double(), MAX_V, MAX_W, sigma, seed, counter, clip=False)
            above, below = raw > hi + bound, raw < lo - bound
            assert torch.equal(got[above], hi.float().expand(n, 2)[above])
            assert torch.equal(got[below], lo.float().expand(n, 2)[below])
            if sigma == 0.0:        # +-inf and +-100 saturate both heads exactly
                sat = lg.isinf() | (lg.abs() == 100)
                assert torch.equal(got[sat], torch.where(lg[sat] > 0, hi.float().expand(n, 2)[sat],
                                                         lo.float().expand(n, 2)[sat]))
                assert int(sat.sum()) == 8
    rows = 1 << 20
    lg = torch.stack([torch.full((rows,), -math.inf), torch.zeros(rows)], 1).cuda().contiguous()
    big = float(np.float32(1e9))
    for seed, counter in KEYS[2:]:
        got = _tail(lg, big, big, 1.0, seed, counter)
        want, bound = A.act(None, lg.double(), big, big, 1.0, seed, counter)
        worst["noise alone"] = max(worst.get("noise alone", 0.0), _check(got, want, bound, ("tail noise", seed, counter)))
        assert float(got.abs().max()) > 4.5                 # the tail of the distribution is in the sample
    print("cn_policy_tail worst error / bound:", {k: "%.3g" % v for k, v in worst.items()})


def _rollout(world, N, T, seed):
    """cn_rollout_policy on `world` for T periods; every action compared with the float64 actor on the observation the kernel
    read (obs0 at t = 0, the trajectory's obs[t - 1] after), noise keyed by counter c + t."""
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    cfg = Config(n_envs=N, max_steps=9, seed=seed, ped_cycle_ms=1400, **world)
    env = VecEnv(cfg)
    env.reset()
    torch.cuda.synchronize()
    D, K = env.D, env.K
    obs0 = env.obs.clone()
    p = make_actor(D, seed, obs0)
    agent = Agent(obs_dim=D, device="cuda:0", seed=seed, memory_size=16)
    with torch.no_grad():
        for i, k in ((1, "1"), (2, "2"), (3, "3")):
            getattr(agent.actor, "linear" + k).weight.copy_(p["w%d" % i].float())
            getattr(agent.actor, "linear" + k).bias.copy_(p["b%d" % i].float())
    agent.explore_sigma = SIGMA
    agent.sync_fused_weights()
    nseed, calls = KEYS[3][0], KEYS[3][1]
    agent.set_noise_state(nseed, calls)
    traj = dict(action=torch.zeros((T, N, 2), device="cuda"), obs=torch.zeros((T, N, D), device="cuda"),
                reward=torch.zeros((T, N), device="cuda"), done=torch.zeros((T, N), dtype=torch.uint8, device="cuda"),
                topk_idx=torch.zeros((T, N, K), dtype=torch.int32, device="cuda"))
    env.rollout_policy(agent, T, traj=traj, obs0=obs0)
    torch.cuda.synchronize()
    worst = 0.0
    for t in range(T):
        o = obs0 if t == 0 else traj["obs"][t - 1]
        want, bound = A.act(p, o.double(), MAX_V, MAX_W, SIGMA, nseed, calls + 1 + t)
        worst = max(worst, _check(traj["action"][t], want, bound, (world, t)))
    return env, worst


def test_rollout_policy_720_rays():
    """The s720 world (100 pedestrians, 720 rays, K = 8: obs_dim 758, Dp 768, 8 environments per policy workgroup)."""
    env, worst = _rollout(dict(n_peds=100, n_rays=720, room_half=2.40), 76, 6, 61)
    assert env.D == 758 and env.kernel_name("policy") == "cn_policy_kernel_s720"
    print("cn_rollout_policy s720: %.3g of the bound" % worst)


def test_rollout_policy_widest_world():
    """WIDEST_WORLD (965 rays, K = 16, no pedestrians: obs_dim 1035, Dp 1056); 1025 rays and 966 rays with K = 16 are refused
    for LDS."""
    import crowdnav
    from crowdnav import Config
    from crowdnav.env import VecEnv
    from crowdnav.td3 import Agent
    for rays, D in ((1025, 1095), (WIDEST_WORLD["n_rays"] + 1, 1036)):      # 1025 rays and one ray more than WIDEST_WORLD
        wide = VecEnv(Config(n_envs=16, n_rays=rays, k_obstacles=16, n_peds=0, room_half=3.0))
        wide.reset()
        assert wide.D == D
        agent = Agent(obs_dim=wide.D, device="cuda:0", seed=0, memory_size=16)
        with pytest.raises(crowdnav.CrowdNavError, match="fit one CU's LDS"):
            wide.rollout_policy(agent, 1)
    env, worst = _rollout(WIDEST_WORLD, 40, 4, 62)
    assert env.D == 1035 and env.kernel_name("policy") == "cn_policy_kernel"
    print("cn_rollout_policy %s: %.3g of the bound" % (WIDEST_WORLD, worst))


def test_wrong_references_are_rejected():
    """Each wrong variant of the reference breaks the bound at least once against the kernel's output: 32 observation columns
    zeroed in the second staging chunk (width 758), the last 32-input block dropped, the noise keyed by row % 16, sin and cos
    exchanged, the counter off by one."""
    D = 758
    obs, p, pk = _case(D, 1000, 7)
    seed, counter = KEYS[3]
    got = pk.forward(obs, SIGMA, seed, counter)
    want, bound = A.act(p, obs.double(), MAX_V, MAX_W, SIGMA, seed, counter)
    _check(got, want, bound, "the right reference")
    o2 = obs.double().clone()
    o2[:, 512:544] = 0
    o3 = obs.double().clone()
    o3[:, (D + 31) // 32 * 32 - 32:] = 0
    worst = {}
    for name, o, mut in (("chunk 2 columns 512-543 zeroed", o2, None), ("last 32-input block dropped", o3, None),
                         ("noise keyed by row % 16", obs.double(), "row_mod16"), ("sin and cos swapped", obs.double(), "swap"),
                         ("counter + 1", obs.double(), "counter+1")):
        w_, b_ = A.act(p, o, MAX_V, MAX_W, SIGMA, seed, counter, mutation=mut)
        worst[name] = worst_ratio(got, w_, b_)
        assert worst[name] > 1.0, (name, worst[name])
    print("rejected wrong references (worst error / bound):", {k: "%.3g" % v for k, v in worst.items()})
