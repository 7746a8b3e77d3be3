"""The fused learners' replay sampling and TD3's target-policy noise (td3_prep_kernel in csrc/crowdnav_gemm.hip, the replay path of
cn_td3_update and cn_ddpg_update) as a CPU statement: exact integers for the indices, float64 for the noise, and the allowance the
GPU tests hold the float32 noise to.  No kernel code and no libcrowdnav: numpy uint64 for the generator (actor_f64's).

The operation, for row m of the handle's update number c (0 at create, one more after every update of any kind):
  h     = mix64(mix64(seed ^ mix64(c)) ^ (uint32) m)                 (actor_f64.noise_key: the exploration noise's hash)
  index = h % max(size, 1)                  size = *replay_size_dev when the update runs; 0 and negative sizes count as 1
  h'    = the same hash with the counter c ^ 0x5bd1e995
  u1 = ((h' >> 40) + 1) 2^-24 in (0, 1],  u2 = ((h' >> 8) & 0xffffff) 2^-24 in [0, 1)   (exact in float32: actor_f64.uniforms)
  z  = (r cos a, r sin a),  r = sqrt(-2 ln u1),  a = fl32(6.2831855f u2)
  noise = clip(z noise_std, -noise_clip, noise_clip)                 (TD3:240-242: the scale first, then the clip)
The angle is reproduced as the kernel rounds it: 6.28318530718f is 6.2831855f, u2 is exact, and the build's -ffp-contract=off
leaves one v_mul_f32 -- so `a` is the float32 product, and sin / cos are taken of that float32 value.

Allowance per element (U = 2^-24; 1 ulp of a normal float32 x is at most 2U |x|).  The prep kernel calls OCML's full-precision
logf / sqrtf / sinf / cosf: its gfx950 code has no v_sin_f32 / v_cos_f32, the argument reduction uses v_alignbit_b32, and ln is
v_log_f32 scaled by ln 2 in extended precision.  HIP documents these at 1 (logf), 2 (sinf, cosf) and 1 (sqrtf) ulp; sqrtf here
is v_sqrt_f32 followed by the two fma corrections that round it correctly, so it is taken at 0.5 ulp.  Relative to the float64
r |cos a| (or r |sin a|):
  ln u1 within 2U, so -2 ln u1 within 2U and its square root within U;  sqrtf's rounding U     -> r within 2U
  cosf / sinf of the float32 angle within 4U;  r * c one rounding U;  * noise_std one rounding U
  = 8U, times SLACK for the products of these terms.  The clip is exact and 1-Lipschitz: it never widens an error.
Where the statement is exactly zero (u1 = 1, u2 = 0 in the sine column, noise_std = 0, noise_clip = 0) the allowance is zero.
Nobody has measured how close the device comes to these figures; the HIP ulp figures are the library's documented maxima, not a
measurement on the MI355X.  The GPU tests print the worst error / allowance they see (0.58 over 2 x 2 x 64 x 4096 x 2 elements
of the two settings that draw noise, when this was written)."""
import math

import numpy as np

from actor_f64 import MASK64, mix64, noise_key, uniforms

U = 2.0 ** -24
NOISE_XOR = 0x5BD1E995          # the noise key: counter ^ this
TWO_PI_F32 = np.float32(6.28318530718)      # == 6.2831855f
E_R = 2 * U                     # r: logf (1 ulp, halved by the square root) + sqrtf's rounding
E_SC = 4 * U                    # sinf / cosf: 2 ulp
E_NOISE = E_R + E_SC + 2 * U    # + the roundings of r * c and of * noise_std
SLACK = 1.0 + 2.0 ** -8

INDEX_VARIANTS = ("counter+1", "counter-1", "row+1", "hi32", "capacity")
NOISE_VARIANTS = ("sincos", "index_key", "u_swap", "scale_after_clip", "clip_at_std")


def live(size):
    """The divisor the kernel uses: max(size, 1) (an int64 on the device; 0 and negatives are taken as 1)."""
    return max(int(size), 1)


def indices(seed, counter, B, size, variant=None, capacity=None, rows=None):
    """Ring rows of batch rows 0 .. B-1 (or of the listed `rows`) of update `counter` (int64).  variant: one of INDEX_VARIANTS, a wrong statement the
    tests must be able to tell apart -- the counter or the row off by one, the high word of the hash instead of all of it, the
    ring's capacity (`capacity`) instead of its live size."""
    rows = np.arange(B, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    c = int(counter) + {"counter+1": 1, "counter-1": -1}.get(variant, 0)
    if variant == "row+1":
        rows = rows + 1
    h = noise_key(seed, c & MASK64, rows)
    if variant == "hi32":
        h = h >> np.uint64(32)
    n = live(capacity if variant == "capacity" else size)
    return (h % np.uint64(n)).astype(np.int64)


def noise_hash(seed, counter, B, rows=None):
    return noise_key(seed, (int(counter) ^ NOISE_XOR) & MASK64, np.arange(B) if rows is None else rows)


def angle_f32(u2):
    """fl32(6.2831855f u2) as float64 (u2 is exact in float32)."""
    return (np.asarray(u2, dtype=np.float64).astype(np.float32) * TWO_PI_F32).astype(np.float64)


def target_noise(seed, counter, B, std, clip, variant=None):
    """(noise [B, 2] float64, allowance [B, 2]) of update `counter`.  std and clip are taken as the float32 values the kernel
    receives.  variant: one of NOISE_VARIANTS -- sin and cos exchanged, the index's key (no 0x5bd1e995), u1 and u2 drawn from
    each other's bits, the scale after the clip, the clip at noise_std."""
    std, clip = float(np.float32(std)), float(np.float32(clip))
    if variant == "index_key":
        h = noise_key(seed, int(counter) & MASK64, np.arange(B))
    else:
        h = noise_hash(seed, counter, B)
    if variant == "u_swap":
        u1 = (((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0) * U
        u2 = (h >> np.uint64(40)).astype(np.float64) * U
    else:
        u1, u2 = uniforms(h)
    r = np.sqrt(-2.0 * np.log(u1))
    a = angle_f32(u2)
    sc = np.stack([np.cos(a), np.sin(a)], 1)
    if variant == "sincos":
        sc = sc[:, ::-1]
    z = r[:, None] * sc
    if variant == "scale_after_clip":
        out = np.clip(z, -clip, clip) * std
    elif variant == "clip_at_std":
        out = np.clip(z * std, -std, std)
    else:
        out = np.clip(z * std, -clip, clip)
    bound = E_NOISE * SLACK * std * np.abs(z)
    return out, bound


# ---- seeds that put the generator's extremes on known (counter, row) ----------------------------------------------------
EXTREMES = {                    # name: (which 24-bit field of the noise hash, its value)
    "u1_min": (40, 0),                      # u1 = 2^-24: the largest r, sqrt(48 ln 2) = 5.77
    "u1_one": (40, 0xFFFFFF),               # u1 = 1: r = 0, the noise is exactly zero
    "u2_zero": (8, 0),                      # a = 0: the sine column is exactly zero
    "u2_quarter": (8, 1 << 22),             # a = fl32(pi / 2): the cosine column is ~4e-8 r
    "u2_half": (8, 1 << 23),                # a = fl32(pi): the sine column is ~9e-8 r
    "u2_three_quarter": (8, 3 << 22),       # a = fl32(3 pi / 2): the cosine column is small
    "u2_max": (8, (1 << 24) - 1),           # u2 = 1 - 2^-24: the sine column is ~ -4e-7 r
}


def field(h, shift):
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(shift)) & np.uint64(0xFFFFFF)


def find_extreme_seeds(B=4096, counters=64, first_seed=1, max_seeds=20000):
    """{name: (seed, counter, row)} for every EXTREMES entry: the smallest seed >= first_seed (then the smallest counter, then
    row) whose noise hash at some counter < `counters` and row < B has the field at the value.  Deterministic; about a second."""
    found = {}
    rows = np.arange(B, dtype=np.uint64)
    cs = [(c ^ NOISE_XOR) & MASK64 for c in range(counters)]
    for seed in range(first_seed, first_seed + max_seeds):
        base = mix64(np.uint64(seed) ^ mix64(np.array(cs, dtype=np.uint64)))
        h = mix64(base[:, None] ^ rows[None, :])
        for name, (shift, val) in EXTREMES.items():
            if name in found:
                continue
            hit = np.argwhere(field(h, shift) == np.uint64(val))
            if hit.size:
                c, m = hit[0]
                found[name] = (seed, int(c), int(m))
        if len(found) == len(EXTREMES):
            return found
    raise RuntimeError("no seed below %d places every extreme" % (first_seed + max_seeds))


KNOWN_BITS = 0xFFFFFF00FFFFFF00         # what the exploration noise reads of its hash: u1 from bits 40..63, u2 from bits 8..31


def index_window(seed, counter, m, size):
    """What the exploration noise of environment row m under the key (seed, counter) reveals about batch row m of the learner's
    update number `counter` when the learner has the same seed (crowdnav.td3.Agent passes its exploration seed): they share the
    hash h, the noise fixes h's bits 8..31 and 40..63, so the index is one of the h % size over the 2^16 values of bits 0..7 and
    32..39.  Returns that candidate set."""
    h = int(noise_key(seed, counter, [m])[0]) & KNOWN_BITS
    return {(h + j + (k << 32)) % live(size) for j in range(256) for k in range(256)}


def r_max():
    return math.sqrt(-2.0 * math.log(U))


# ---- the GPU test's plan (tests/test_gpu_sampling_f64.py), here so that the CPU tests can show it tells the variants apart ----
LIVE_SIZES = (1, 2, 3, 37, 63, 64, 65, 4096, 5003, 65536, (1 << 20) - 1, 1_000_000, (1 << 24) + 1)
DEGENERATE_SIZES = (0, -1, -(1 << 63))          # *size_dev values the kernel takes as 1
CAPACITY = (1 << 24) + 4099                     # the index test's ring (rows encode their slot)
BATCHES = (1, 129, 4096)
INDEX_SEEDS = (0, MASK64, 0x6A09E667F3BCC908)
NOISE_SEEDS = (3, 0xBB67AE8584CAA73B)
NOISE_SETTINGS = ((0.2, 0.5), (1.0, 100.0), (0.25, 0.0), (0.0, 0.5))     # (noise_std, noise_clip)
NOISE_B, NOISE_UPDATES = 4096, 64


def index_plan():
    """The *size_dev value of each update of one handle in the index test: every live size twice, then the degenerate ones."""
    return [s for s in LIVE_SIZES for _ in range(2)] + list(DEGENERATE_SIZES)
