"""CPU checks of tests/actor_f64.py, the float64 statement the GPU tests hold the fused actor and cn_policy_tail to: the generator
restatement against splitmix64's known answer and the kernel's key layout, the uniforms' edge values, and the bound (non-negative,
growing with the width, and met by a float32 evaluation of the same actor)."""
import math

import numpy as np
import torch

import actor_f64 as A


def test_mix64_is_splitmix64():
    """splitmix64 seeded with 0 yields 0xE220A8397B1DCDAF first: its state advances by the golden gamma, then the finaliser,
    which is what mix64 does to 0.  The next two outputs follow from the state 2 x and 3 x gamma."""
    g = 0x9E3779B97F4A7C15
    got = A.mix64(np.array([0, g, 2 * g & A.MASK64], dtype=np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_noise_key_layout():
    """mix64(mix64(seed ^ mix64(counter)) ^ (uint32) row), with all 64 bits of seed and counter and the row taken mod 2^32."""
    seed, counter = (1 << 63) | 12345, (1 << 40) + 3
    rows = np.array([0, 1, 65536, (1 << 31) - 1])
    inner = int(A.mix64(np.array([seed ^ int(A.mix64(np.array([counter], dtype=np.uint64))[0])], dtype=np.uint64))[0])
    want = A.mix64(np.array([inner ^ int(r) for r in rows], dtype=np.uint64))
    assert np.array_equal(A.noise_key(seed, counter, rows), want)
    assert np.array_equal(A.noise_key(seed, counter, rows + (1 << 32)), want)
    # every bit of the seed and of the counter reaches the key
    for s, c in ((seed ^ (1 << 63), counter), (seed, counter ^ (1 << 40)), (seed ^ 1, counter), (seed, counter ^ (1 << 32))):
        assert not np.array_equal(A.noise_key(s, c, rows), want)


def test_uniform_edge_values():
    """u1 = (k + 1) 2^-24 over k = h >> 40 and u2 = k' 2^-24 over k' = (h >> 8) & 0xffffff: u1's smallest value is 2^-24, its
    largest exactly 1 (r = 0), u2 runs from 0 to 1 - 2^-24; both are the float32 values the kernel computes, and 1.0f /
    16777217.0f is exactly 2^-24."""
    assert np.float32(1.0) / np.float32(16777217.0) == np.float32(2.0 ** -24)
    h = np.array([0, (1 << 64) - 1, 0xFFFFFF << 40, 0xFFFFFF << 8, 0xFF], dtype=np.uint64)
    u1, u2 = A.uniforms(h)
    assert u1.tolist() == [2.0 ** -24, 1.0, 1.0, 2.0 ** -24, 2.0 ** -24]
    assert u2.tolist() == [0.0, 1 - 2.0 ** -24, 0.0, 1 - 2.0 ** -24, 0.0]
    assert all(float(np.float32(x)) == x for x in np.concatenate([u1, u2]))          # exact float32 values
    r, c, s = A.box_muller(u1, u2)
    assert r[1] == 0.0 and abs(r[0] - math.sqrt(48 * math.log(2))) < 1e-12 and c[0] == 1.0 and s[0] == 0.0
    nv, nw, _, _ = A.noise(0, 1, np.arange(8))
    nv2, nw2, _, _ = A.noise(0, 1, np.arange(8), swap=True)
    assert np.array_equal(nv, nw2) and np.array_equal(nw, nv2)


def _actor(D, seed):
    g = torch.Generator().manual_seed(seed)

    def lin(i, o):
        k = 1.0 / math.sqrt(i)
        return [((torch.rand(s, generator=g, dtype=torch.float64) * 2 - 1) * k).float().double() for s in ((o, i), (o,))]
    p = dict(zip(("w1", "b1", "w2", "b2", "w3", "b3"), lin(D, 256) + lin(256, 256) + lin(256, 2)))
    p["w3"] = (p["w3"] * 8).float().double()
    return p, torch.randn((64, D), generator=g).double()


def test_bound_is_non_negative_grows_with_the_width_and_holds_for_float32():
    """The logit bound and the action bound are non-negative and finite, grow with the width (N and M both do), and a float32
    evaluation of the same actor (torch's CPU order, an order of its own) lies within them."""
    prev = None
    for D in (1, 33, 398, 758, 1095):
        p, obs = _actor(D, D)
        lg, dl = A.logits_and_bound(p, obs)
        assert bool((dl >= 0).all() and torch.isfinite(dl).all())
        act, bound = A.act(p, obs, 0.22, 2.0)
        assert bool((bound > 0).all() and torch.isfinite(bound).all())
        med = float(dl.median())
        if prev is not None:
            assert med > prev
        prev = med
        assert A.chain_length((D + 31) // 32 * 32) >= D + 512
        p32 = {k: v.float() for k, v in p.items()}
        h = torch.relu(obs.float() @ p32["w1"].T + p32["b1"])
        h = torch.relu(h @ p32["w2"].T + p32["b2"])
        l32 = h @ p32["w3"].T + p32["b3"]
        assert float(((l32.double() - lg).abs() / dl).max()) <= 1.0
        a32 = torch.stack([torch.sigmoid(l32[:, 0]) * np.float32(0.22), torch.tanh(l32[:, 1]) * np.float32(2.0)], 1)
        assert float(((a32.double() - act).abs() / bound).max()) <= 1.0


def test_heads_at_the_extremes_and_the_clip():
    """+-inf logits give the exact clip bounds with no NaN in the allowance; the unclipped value is returned on request."""
    lg = torch.tensor([[math.inf, -math.inf], [-math.inf, math.inf], [0.0, 0.0], [-100.0, 100.0]], dtype=torch.float64)
    act, bound = A.act(None, lg, 0.22, 2.0)
    assert act.tolist()[:2] == [[0.22, -2.0], [0.0, 2.0]] and bool(torch.isfinite(bound).all())
    assert float(bound[2, 1]) == 0.0 and float(bound[0, 0]) > 0          # tanh(0) = 0 exactly in the kernel's polynomial
    raw, _ = A.act(None, lg, 0.22, 2.0, sigma=1.0, seed=3, counter=9, clip=False)
    cl, _ = A.act(None, lg, 0.22, 2.0, sigma=1.0, seed=3, counter=9)
    assert torch.equal(cl, torch.maximum(torch.minimum(raw, torch.tensor([0.22, 2.0], dtype=torch.float64)),
                                         torch.tensor([0.0, -2.0], dtype=torch.float64)))
