"""A float64 statement of the fused TD3 actor (actor_tile in csrc/crowdnav_actor.h: cn_actor_forward, csrc/crowdnav_actor.hip, and the policy
phase of cn_rollout_policy) and of the output stage cn_policy_tail, with the error bounds the GPU tests hold the float32 kernels to.
No kernel code and no libcrowdnav: torch float64 for the network, numpy uint64 for the generator.

The operation (crowdnav.td3.Actor, Agent.act):
  logits = linear3(relu(linear2(relu(linear1(obs)))))
  v = max_v sigmoid(l0) + sigma n_v,  w = max_w tanh(l1) + sigma n_w,  v clipped to [0, max_v], w to [-max_w, max_w]
  (n_v, n_w) = (r cos(2 pi u2), r sin(2 pi u2)), r = sqrt(-2 ln u1)                          (Box-Muller; v takes cos)
  h  = mix64(mix64(seed ^ mix64(counter)) ^ (uint32) row)        (mix64 = splitmix64's finaliser, crowdnav_device.h cn_mix64)
  u1 = ((h >> 40) + 1) 2^-24 in (0, 1],  u2 = ((h >> 8) & 0xffffff) 2^-24 in [0, 1)
  The kernel's float32 expressions give these u1, u2 exactly: the 24-bit integers (+ 1) are exact in float32, and the literal
  1.0f / 16777217.0f is exactly 2^-24 because 16777217.0f rounds to 16777216.  `row` is the global row of the batch (cn_actor_forward)
  or the environment index (cn_rollout_policy, which keys period t with counter + t).

Bounds (u = 2^-24).  Every allowance below is a bound on |kernel - float64 statement| per action element.
- Network: the strict forward bound gamma_N M, gamma_N = N u / (1 - N u), N = chain_length(Dp) = Dp + 2 x 256 + 32 roundings
  (linear1's Dp-long fma chain on the matrix cores, linear2's 256, linear3's per-lane pair + 4 DPP adds + 8 wave partials < 256,
  three bias adds; the spare covers them).  M is the logits' MAGNITUDE: the same network evaluated on |W|, |b|, |obs|.  ReLU is
  1-Lipschitz, so the bound survives a mask that flips in float32 and needs no bias margins -- which is what lets the same check
  run on the observations the simulator writes.  A hidden unit counts as live in M if its pre-activation lies within its own
  bound of zero (a unit that turns positive in float32 still feeds the next layer).  The logit bound reaches the actions through
  the largest head derivative over [l - dl, l + dl].
- Heads, from the instructions of the gfx950 code objects of cn_actor_kernel, cn_policy_kernel* and cn_policy_tail_kernel
  (llvm-objdump of the build's device code):
  * sigmoid: max_v / (1.0f + __expf(-l)) is v_mul_f32(l, -log2e_f32), v_exp_f32, v_add_f32 1.0, and a correctly rounded
    v_div_scale / v_div_fmas / v_div_fixup division.  The product rounds (u) and log2e_f32 is off by 1.34e-8 relative, so
    2^t carries |l| (u + 1.34e-8) + E_EXP relative error -- it grows with |l| -- and v
    max_v s ((1 - s)(|l| (u + 1.34e-8) + E_EXP) + 2 u).  Where 2^t overflows or max_v / (1 + e) underflows the kernel returns 0
    (or a denormal): the absolute floor TINY covers the float64 value there (< 1e-38).
  * tanhf (OCML): for |l| >= 0.625, 1 - 2 v_rcp_f32(1 + v_exp_f32(2 |l| log2e)) with log2e split into two floats (exact
    argument), then copysign: absolute error <= 0.46 (E_EXP + E_RCP + u) + u there, where |tanh| >= 0.55; for |l| < 0.625
    l + l^3 P(l^2) by fma (exactly 0 at l = 0).  Both are within E_TANH |tanh l|; then u |w| for the product with max_w.
  * noise: __logf is v_log_f32 scaled by ln 2 in extended precision (v_mul + v_fma + v_fmamk); ln u1 within E_LOG relative; -2 x
    exact; sqrtf is correctly rounded (v_sqrt_f32 + two v_fma corrections): r within E_LOG / 2 + u relative.  __sincosf is
    v_sin_f32 / v_cos_f32 of the revolution count fl(fl(u2 x 6.2831855f) x 0.15915494f), which is within 2 u + 1.3e-8 relative of
    u2 (so 2 pi 2.25 u u2 absolute in the angle) and the hardware adds E_SC absolute.  sigma r rounds twice (2 u), adding the
    noise to the head once more (u |v + n|).  The clip is exact and 1-Lipschitz: it never widens an error.
- E_EXP, E_TANH, E_LOG and E_SC: the instruction set reference gives no accuracy figure for v_exp_f32 / v_log_f32 / v_rcp_f32 /
  v_sin_f32 / v_cos_f32 that this module could cite, so these four rest on numbers MEASURED on the MI355X with cn_policy_tail.
  Heads on 2^22 logits over [-40, 40]: the exponential's own error came to 0.2 u relative (allowed E_EXP = 4 u), tanhf's to
  2.3 u relative (allowed E_TANH = 4 u); the sigmoid head then reaches 0.86 of its allowance, most of it the |l| term.  The
  noise alone (v's head at 0 by l0 = -inf, w's at tanh(0) = 0) on 2^22 rows under two keys: |error| / r up to 4.1e-7 where
  |cos| or |sin| < 0.05 (most of it the argument's rounding; E_SC = 2^-21 = 4.8e-7 comes on top), 5.3 u relative where they
  exceed 0.95, and 0.36 of the whole noise allowance at worst.  The measurements do not separate the logarithm from sin / cos:
  E_LOG = 8 u is the allowance they were checked with.  cn_actor_kernel, cn_policy_kernel and cn_policy_tail_kernel carry the
  same instruction sequences for the heads and the noise."""
import math

import numpy as np
import torch

from td3_f64 import U, actor_fwd

SPARE = 32                   # roundings beyond Dp + 2 x 256: bias adds, linear3's lane pair, DPP scan and wave partials
LOG2E_ERR = 1.34e-8          # |log2e_f32 / log2e - 1|, 0x3fb8aa3b
REV_ERR = 2.25 * U           # revolution count fl(fl(u2 6.2831855f) 0.15915494f) against u2: two roundings + 1.26e-8 of constants
E_EXP = 4 * U                # v_exp_f32 relative (these four: measured, see the docstring)
E_TANH = 4 * U               # tanhf relative
E_LOG = 8 * U                # __logf relative
E_SC = 2.0 ** -21            # v_sin_f32 / v_cos_f32 absolute
TINY = 2.0 ** -126           # smallest normal float32: underflow / flush of the sigmoid head
SLACK = 1.0 + 2.0 ** -8      # first-order error terms: products of two allowances are below this factor

MASK64 = (1 << 64) - 1
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def chain_length(Dp):
    return Dp + 2 * 256 + SPARE


def gamma(N):
    return N * U / (1.0 - N * U)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def mix64(z):
    """splitmix64's finaliser (cn_mix64) on a uint64 array, wrapping like the device's 64-bit integers."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def noise_key(seed, counter, rows):
    """The per-row 64-bit hash: mix64(mix64(seed ^ mix64(counter)) ^ (uint32) row); seed and counter are Python ints < 2^64."""
    base = mix64(np.array([int(seed) & MASK64], dtype=np.uint64) ^ mix64(np.array([int(counter) & MASK64], dtype=np.uint64)))
    r = np.asarray(rows, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return mix64(base ^ r)


def uniforms(h):
    """(u1, u2) of a hash, exactly the kernel's float32 values: u1 = (k + 1) 2^-24 in (0, 1], u2 = k' 2^-24 in [0, 1)."""
    h = np.asarray(h, dtype=np.uint64)
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def box_muller(u1, u2):
    """(r, cos(2 pi u2), sin(2 pi u2)) in float64."""
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * math.pi * u2
    return r, np.cos(a), np.sin(a)


def noise(seed, counter, rows, swap=False):
    """float64 (n_v, n_w, r, u2) of the listed rows (unit sigma); swap: the wrong variant with sin and cos exchanged."""
    u1, u2 = uniforms(noise_key(seed, counter, rows))
    r, c, s = box_muller(u1, u2)
    if swap:
        c, s = s, c
    return r * c, r * s, r, u2


def noise_allowance(sigma, r, sc, u2):
    """|float32 sigma n - sigma r sc| allowed for one component (before the add to the head), sc = its cos or sin."""
    return sigma * r * (np.abs(sc) * (E_LOG / 2 + 3 * U) + 2 * math.pi * REV_ERR * u2 + E_SC)


# ---- heads -----------------------------------------------------------------------------------------------------------------
def heads(logits, max_v, max_w):
    """(v, w) in float64 and the heads' own allowances for exact float32 logits (logits [n, 2] float64)."""
    l0, l1 = logits[:, 0], logits[:, 1]
    s = torch.sigmoid(l0)
    v = max_v * s
    w = max_w * torch.tanh(l1)
    fin = torch.isfinite(l0)
    grow = torch.where(fin, (1 - s) * l0.abs().nan_to_num(0.0), torch.zeros_like(l0))    # (1 - s)|l|: 0 at l = +-inf
    a_v = max_v * s * (grow * (U + LOG2E_ERR) + (1 - s) * E_EXP + 2 * U) + TINY
    a_w = (E_TANH + U) * w.abs()
    return torch.stack([v, w], 1), torch.stack([a_v, a_w], 1)


def _head_slope(logits, dl, max_v, max_w):
    """The largest |d action / d logit| over [l - dl, l + dl] (both heads peak at 0 and fall off monotonically on each side)."""
    near = torch.where(logits.abs() <= dl, torch.zeros_like(logits), logits.abs() - dl)
    s = torch.sigmoid(near[:, 0])
    t = torch.tanh(near[:, 1])
    return torch.stack([max_v * s * (1 - s), max_w * (1 - t * t)], 1)


# ---- the network -----------------------------------------------------------------------------------------------------------
def logits_and_bound(p, obs):
    """float64 logits of the actor p (td3_f64 names: w1 [256, D], b1, w2, b2, w3 [2, 256], b3) on obs [n, D], and their bound
    gamma_N M with the relaxed live masks (docstring).  Dp = D rounded up to 32."""
    D = obs.shape[1]
    N = chain_length((D + 31) // 32 * 32)
    g = gamma(N)
    f = actor_fwd(p, obs, dict(max_v=1.0, max_w=1.0), with_mag=False)
    xm = obs.abs()
    m1 = xm @ p["w1"].abs().T + p["b1"].abs()
    mh1 = m1 * (f["z1"] > -g * m1)
    m2 = mh1 @ p["w2"].abs().T + p["b2"].abs()
    mh2 = m2 * (f["z2"] > -g * m2)
    m_out = mh2 @ p["w3"].abs().T + p["b3"].abs()
    return f["logits"], g * m_out


def act(p, obs, max_v, max_w, sigma=0.0, seed=0, counter=0, rows=None, mutation=None, clip=True):
    """The actions [n, 2] of the actor (or of cn_policy_tail when p is None and obs are the logits) in float64, and the bound.
    rows: the generator's rows (default 0..n-1).  mutation (the wrong variants the tests must reject): "row_mod16" keys the noise
    by row % 16, "swap" exchanges sin and cos, "counter+1" shifts the counter; obs-side mutations are the caller's.
    clip=False: the value before the clip."""
    if p is None:
        lg, dl = obs, torch.zeros_like(obs)
    else:
        lg, dl = logits_and_bound(p, obs)
    val, allow = heads(lg, max_v, max_w)
    bound = allow + _head_slope(lg, dl, max_v, max_w) * dl
    if sigma > 0:
        n = lg.shape[0]
        r_ = np.arange(n) if rows is None else np.asarray(rows)
        if mutation == "row_mod16":
            r_ = r_ % 16
        ctr = counter + 1 if mutation == "counter+1" else counter
        nv, nw, r, u2 = noise(seed, ctr, r_, swap=mutation == "swap")
        nz = torch.from_numpy(np.stack([nv, nw], 1)).to(lg.device) * sigma
        rr = np.stack([r, r], 1)
        sc = np.stack([nv, nw], 1) / np.where(rr > 0, rr, 1.0)
        na = torch.from_numpy(noise_allowance(sigma, rr, sc, np.stack([u2, u2], 1))).to(lg.device)
        val = val + nz
        bound = bound + na + U * val.abs()
    bound = bound * SLACK
    if not clip:
        return val, bound
    lo = torch.tensor([0.0, -max_w], dtype=val.dtype, device=val.device)
    hi = torch.tensor([max_v, max_w], dtype=val.dtype, device=val.device)
    return torch.maximum(torch.minimum(val, hi), lo), bound
