"""Python's and numpy's own statements of the device arithmetic in csrc/crowdnav_device.h -- the roundings, the constant
divisions, the IoU of two squares, the bare-instruction helpers and the wave helpers -- and the input sets the tests of that
arithmetic run on (tests/test_device_math_helpers.py on the CPU, tests/test_gpu_device_math.py on the device).  Plain Python and
numpy: nothing here comes from the oracle or from the kernels.

References
- round(x, nd) under Python 3: the builtin (py3_round), cross-checked with Decimal(x).quantize(ROUND_HALF_EVEN).
- round(x, nd) under Python 2.7: Decimal(x).quantize(ROUND_HALF_UP) on the exact binary value (py27_round) -- floatobject.c's
  _Py_double_round contract: correctly rounded, an exact tie goes away from zero.  Both keep the sign of x on a zero result.
- np.around / round(np.float64(x), nd): numpy (np_around, np64_round).  round(np.float64, 2) as the environment meets it
  (round_np64): numpy under Python 3, the 2.7 builtin under Python 2.7.
- IoU of two axis-aligned squares (UTL:422-460): the corner sums in float64 as the reference writes them, intersection and
  union as exact rationals of those corners, the quotient rounded once to float64 and then to three decimals (iou3).
- fmin / fmax / clamp / xorsign: numpy; the single-rounding fma: exact rationals (fma).
- the wave helpers: numpy over rows of 64 lanes.

Domain.  Inputs are finite (the environment sanitises inf / NaN before it rounds).  The `_t<true>` forms drop their range
guard and hold for |rint(x p)| < 2^31 (ROUND_SMALL).  The guarded forms are exact while |x p| < 2^52 (ROUND_GUARDED): the
float64 product y = x p then still represents every half-integer, so rint(y) can only be misled when y IS a half-integer and
fma(x, p, -y) tells on which side the exact product lies.  From 2^52 on the product itself rounds to an integer and Python,
which rounds the exact decimal expansion of x, can differ by one unit: that is the limit of the domain and nothing is asserted
there.  Every set is fixed by its seed and built once per process."""
import decimal
import fractions
import functools

import numpy as np

P10 = {2: 100.0, 3: 1000.0}
GUARD = 2.0 ** 31                  # |rint(x p)| below it: cn_div1000 / cn_div100 instead of the divide
HALVES = (0.0505, 0.101, 0.03, 0.1)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
_CTX = decimal.Context(prec=1200)  # Decimal(float) is exact whatever the context; quantize must not run out of digits
_F = fractions.Fraction


# ---- rounding ------------------------------------------------------------------------------------------------------------------
def _quantize(x, nd, mode):
    return decimal.Decimal(float(x)).quantize(decimal.Decimal(1).scaleb(-nd), rounding=mode, context=_CTX)


def py3_round(x, nd):
    return np.array([round(float(v), nd) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def py3_round_decimal(x, nd):
    return np.array([float(_quantize(v, nd, decimal.ROUND_HALF_EVEN)) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def py27_round(x, nd):
    return np.array([float(_quantize(v, nd, decimal.ROUND_HALF_UP)) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def py_round(x, nd, py2):
    return py27_round(x, nd) if py2 else py3_round(x, nd)


def round_scaled(x, nd, py2):
    """round(x, nd) 10^nd, the integer cn_round_scaled returns (exact: |x 10^nd| < 2^52); a zero keeps the sign of x"""
    mode = decimal.ROUND_HALF_UP if py2 else decimal.ROUND_HALF_EVEN
    return np.array([float(_quantize(v, nd, mode).scaleb(nd, context=_CTX)) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def np_around(x, nd):
    return np.around(np.asarray(x, dtype=np.float64), nd)


def np64_round(x, nd):
    return np.array([float(round(np.float64(v), nd)) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def round_np64(x, nd, py2):
    return py27_round(x, nd) if py2 else np_around(x, nd)


def _steps(x, k):
    """every x stepped -k .. +k units in the last place"""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _round_parts(nd):
    p = P10[nd]
    rng = np.random.default_rng(20 + nd)
    k = np.arange(-6000, 6001, dtype=np.float64)
    odd = np.arange(-1023, 1024, 2, dtype=np.float64)
    half = 0.5 / p
    g = np.arange(-4, 5, dtype=np.float64)
    frac = np.array([0.0, 0.25, 0.5, 0.75])
    guard = np.array([s * (GUARD + a + f) / p for s in (-1.0, 1.0) for a in g for f in frac])
    parts = dict(
        room=rng.uniform(-3.5, 3.5, 20000),
        near_zero=rng.uniform(-1e-3, 1e-3, 4000),
        near_ties=_steps((k + 0.5) / p, 3),                          # (k + 1/2) / p, 0..3 ulps either way
        ties3=odd / 16.0, ties2=odd / 8.0,                           # exact binary ties at three / two decimals
        to_zero=np.concatenate([-rng.uniform(0.0, half, 2000), _steps(np.array([-half, half]), 3),
                                [-0.0, 0.0, -5e-324, 5e-324, -1e-300, 1e-300, -2.0 ** -1022, -1e-9, 1e-9]]),
        guard=_steps(guard, 2),
    )
    y = np.exp2(rng.uniform(31.0, 52.0, 20000)) * rng.choice([-1.0, 1.0], 20000)
    yh = (np.floor(np.exp2(rng.uniform(31.0, 51.0, 6000))) + 0.5) * rng.choice([-1.0, 1.0], 6000)
    m = (2.0 * np.floor(np.exp2(rng.uniform(10.0, 45.0, 3000))) + 1.0) * rng.choice([-1.0, 1.0], 3000)
    parts["big"] = np.concatenate([y / p, _steps(yh / p, 1), m / (16.0 if nd == 3 else 8.0)])    # products up to 2^52, ties among them
    return parts


@functools.lru_cache(maxsize=None)
def round_guarded(nd):
    """ROUND_GUARDED: every rounding input, |x p| < 2^52 -- the guarded forms' set"""
    x = np.concatenate(list(_round_parts(nd).values()))
    x = x[np.abs(x * P10[nd]) < 2.0 ** 52]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def round_small(nd):
    """ROUND_SMALL: the inputs whose rounded product stays below the guard (|rint(x p)| < 2^31 with a margin of one unit for
    the tie repair) -- the `_t<true>` forms' set, on which they must equal the guarded forms bit for bit"""
    x = round_guarded(nd)
    x = x[np.abs(np.rint(x * P10[nd])) < GUARD - 1.0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tie_layouts(nd):
    """Waves of 64 inputs for the tie ballot of cn_round_scaled: name -> (values, mask of the lanes whose product is exactly a
    half-integer).  The ties alternate between exact ones (odd / 16, odd / 8) and decimal ones whose float64 product lands on
    the half-integer with the exact product beside it (0.0005 x 1000, 2.675 x 100)."""
    p = P10[nd]
    rng = np.random.default_rng(40 + nd)
    exact = np.arange(-1023, 1024, 2, dtype=np.float64) / (16.0 if nd == 3 else 8.0)
    dec = (np.arange(-6000, 6001, dtype=np.float64) + 0.5) / p
    dec = dec[np.abs(dec * p - np.rint(dec * p)) == 0.5]
    dec = dec[~np.isin(dec, exact)]
    ties = np.empty(2 * min(exact.size, dec.size))
    ties[0::2] = rng.permutation(exact)[:ties.size // 2]; ties[1::2] = rng.permutation(dec)[:ties.size // 2]

    def fill(n):
        v = np.round(rng.uniform(-3.5, 3.5, n), 4)
        y = v * p
        v[np.abs(y - np.rint(y)) > 0.4] += 0.3 / p          # nowhere near a half
        return v
    out = {}
    for name, waves, lanes in (("lane0", 1, [(0, 0)]), ("lane63", 1, [(0, 63)]), ("one_lane_of_one_wave", 5, [(2, 37)]),
                               ("all", 3, [(w, l) for w in range(3) for l in range(64)]), ("none", 2, []),
                               ("two_in_the_ragged_last_wave", 2, [(1, 0), (1, 40)])):
        v = fill(64 * waves).reshape(waves, 64)
        for j, (w, l) in enumerate(lanes):
            v[w, l] = ties[j % ties.size]
        v = v.ravel()
        if name == "two_in_the_ragged_last_wave":
            v = v[:64 + 41]                                  # the tie ballot under a partial exec mask
        m = np.abs(v * p - np.rint(v * p)) == 0.5
        assert int(m.sum()) == len(lanes)
        out[name] = (v, m)
    return out


# ---- constant division ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_set():
    """integers |r| < 2^31: a strided sweep, every |r| <= 10^6, the ends (the exhaustive proof is tools/check_const_div.c)"""
    r = np.concatenate([np.arange(-(2 ** 31 - 1), 2 ** 31, 4099, dtype=np.float64), np.arange(-10 ** 6, 10 ** 6 + 1, dtype=np.float64),
                        [2.0 ** 31 - 1, -(2.0 ** 31 - 1), 2.0 ** 31 - 2]])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def divz_set():
    """cn_div_z(a, b): finite a, b zero (either sign) or normal with a quotient far from the exponent range's ends"""
    rng = np.random.default_rng(31)
    n = 40000
    a = np.concatenate([rng.uniform(-5, 5, n), rng.integers(-4000, 4000, n) / 1000.0])
    a[a == 0.0] = 0.0                      # (cn_div gives +0 for -0 over a positive divisor: equal as numbers, its own note)
    b = np.exp(rng.uniform(np.log(1e-12), np.log(1e12), a.size)) * rng.choice([-1.0, 1.0], a.size)
    b[::7] = 0.0; b[3::14] = -0.0
    a[::35] = 0.0                          # 0 / 0
    return a, b


# ---- IoU (UTL:422-460) ---------------------------------------------------------------------------------------------------------
def iou_terms(ax, ay, bx, by, half):
    """(intersection, union) as exact rationals of the float64 corner sums"""
    ax, ay, bx, by, half = float(ax), float(ay), float(bx), float(by), float(half)
    axp, axm, ayp, aym = ax + half, ax - half, ay + half, ay - half
    bxp, bxm, byp, bym = bx + half, bx - half, by + half, by - half
    ix = _F(min(axp, bxp)) - _F(max(axm, bxm))
    iy = _F(min(ayp, byp)) - _F(max(aym, bym))
    inter = ix * iy if (ix > 0 and iy > 0) else _F(0)
    uni = (_F(axp) - _F(axm)) * (_F(ayp) - _F(aym)) + (_F(bxp) - _F(bxm)) * (_F(byp) - _F(bym)) - inter
    return inter, uni


def iou_ratio(ax, ay, bx, by, half):
    return np.array([float(i / u) for i, u in (iou_terms(*t) for t in zip(ax, ay, bx, by, half))], dtype=np.float64)


def iou3(ax, ay, bx, by, half, py2):
    return py_round(iou_ratio(ax, ay, bx, by, half), 3, py2)


@functools.lru_cache(maxsize=None)
def iou_set():
    """(ax, ay, bx, by, half) for every half in HALVES: centres on thousandths, disjoint / overlapping / touching / identical,
    and two dense sweeps of the overlap ratio through [0.0003, 0.0012] (the 0.0005 tie and the 0.00075 shortcut both lie in it)"""
    rng = np.random.default_rng(33)
    cols = []
    for h in HALVES:
        n = 2500
        p1 = np.round(rng.uniform(-1.3, 1.3, (n, 2)), 3)
        p2 = np.round(p1 + rng.uniform(-2.4 * h, 2.4 * h, (n, 2)), 3)                       # on thousandths: overlapping and disjoint
        cols.append((p1, p2, h))
        q1 = np.round(rng.uniform(-1.3, 1.3, (600, 2)), 3)
        q2 = q1.copy()
        q2[:200, 0] = q1[:200, 0] + 2 * h; q2[:200, 1] += np.round(rng.uniform(-h, h, 200), 3)   # touching along x (ix == 0 or an ulp off)
        q2[200:400, 1] = np.round(q1[200:400, 1] - 2 * h, 3)                                # ... along y, back on thousandths
        cols.append((q1, q2, h))                                                           # rows 400..599: identical boxes
        t = np.linspace(0.0003, 0.0012, 3000)
        s1 = np.round(rng.uniform(-1.3, 1.3, (t.size, 2)), 3)
        s2 = s1.copy()
        s2[:, 0] = s1[:, 0] + (2 * h - 4 * h * t / (1 + t)) * rng.choice([-1.0, 1.0], t.size)   # iy = 2 h: ratio = ix / (4 h - ix)
        cols.append((s1, s2, h))
        w = h * np.sqrt(8 * t / (1 + t))                                                    # ix = iy = w: ratio = w^2 / (8 h^2 - w^2)
        d1 = rng.uniform(-1.3, 1.3, (t.size, 2))
        d2 = d1 + (2 * h - w)[:, None] * rng.choice([-1.0, 1.0], (t.size, 2))
        cols.append((d1, d2, h))
    ax = np.concatenate([c[0][:, 0] for c in cols]); ay = np.concatenate([c[0][:, 1] for c in cols])
    bx = np.concatenate([c[1][:, 0] for c in cols]); by = np.concatenate([c[1][:, 1] for c in cols])
    half = np.concatenate([np.full(len(c[0]), c[2]) for c in cols])
    return ax, ay, bx, by, half


# ---- bare-instruction helpers --------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a b + c rounded once (exact rationals), IEEE signed zeros; finite arguments"""
    a, b, c = float(a), float(b), float(c)
    e = _F(a) * _F(b) + _F(c)
    if e != 0:
        return float(e)
    neg_prod = (np.signbit(a) != np.signbit(b))
    if a * b == 0.0 and c == 0.0:
        return -0.0 if (neg_prod and np.signbit(c)) else 0.0
    return 0.0                                   # x + (-x) under round-to-nearest


@functools.lru_cache(maxsize=None)
def pair_set():
    """(a, b, c): every pair of the specials (signed zeros, infinities, a quiet NaN, ones, tiny and huge), random values, and
    a third operand for the clamp"""
    rng = np.random.default_rng(35)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300, 0.12, 3.5])
    a = np.concatenate([np.repeat(sp, sp.size), rng.uniform(-5, 5, 4000), rng.integers(-4000, 4000, 2000) / 1000.0])
    b = np.concatenate([np.tile(sp, sp.size), rng.uniform(-5, 5, 4000), rng.integers(-4000, 4000, 2000) / 1000.0])
    b[-1000:] = a[-1000:]                        # equal operands
    c = np.concatenate([rng.permutation(np.tile(sp, sp.size)), rng.uniform(-5, 5, 6000)])
    return a, b, c


def sign_defined(a, b):
    """where C's fmin / fmax (numpy's) define the sign of the result: everywhere but on two zeros of opposite sign"""
    return ~((a == 0.0) & (b == 0.0) & (np.signbit(a) != np.signbit(b)))


def xorsign(x, s):
    return (np.asarray(x, dtype=np.float64).view(np.uint64) ^ (np.asarray(s, dtype=np.float64).view(np.uint64) & np.uint64(1 << 63))).view(np.float64)


@functools.lru_cache(maxsize=None)
def fma_set():
    rng = np.random.default_rng(36)
    a = np.concatenate([rng.uniform(-2, 2, 3000), rng.integers(-4000, 4000, 500) / 1000.0, [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.5, 3.0]])
    b = np.concatenate([rng.uniform(-2, 2, 3000), rng.integers(-4000, 4000, 500) / 1000.0, [1.0, 1.0, -1.0, -2.0, 0.5, 0.5, -1.0, 1.0 / 3.0]])
    return a, b


FMA_SCALARS = (-1.0 / 6.0, 0.5, 0.0, -0.0)       # addends of cn_fma_s: a polynomial coefficient, an exactly cancelling one, the zeros


# ---- wave helpers: rows of 64 lanes --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wave_rows_d():
    rng = np.random.default_rng(37)
    rows = []
    for lane in range(64):                       # the minimum in each lane in turn, the maximum 17 lanes on
        r = rng.uniform(-5, 5, 64); r[lane] = -100.0 - lane; r[(lane + 17) % 64] = 100.0 + lane
        rows.append(r)
    rows += [np.full(64, 1.25), np.full(64, -3.0), np.full(64, 0.0), np.full(64, -0.0)]
    for _ in range(4):
        rows.append(rng.choice([0.0, -0.0], 64))
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        r = rng.uniform(-5, 5, 64); r[lane] = np.inf; r[(lane + 5) % 64] = -np.inf; rows.append(r)
        r = rng.uniform(-5, 5, 64); r[lane] = np.inf; rows.append(r)
        r = rng.uniform(-5, 5, 64); r[lane] = -np.inf; rows.append(r)
        r = rng.uniform(-5, 5, 64); r[lane] = np.nan; rows.append(r)             # a quiet NaN in one lane: fmin / fmax skip it
        r = np.full(64, np.inf); r[lane] = 0.6; rows.append(r)                   # one finite range among "no return"
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def wave_rows_i():
    rng = np.random.default_rng(38)
    rows = []
    for lane in range(64):
        r = rng.integers(-1000, 1000, 64); r[lane] = -5000 - lane; r[(lane + 17) % 64] = 5000 + lane
        rows.append(r)
    rows += [np.full(64, 7), np.full(64, 0), np.full(64, -1), np.full(64, INT_MAX), np.full(64, INT_MIN), np.full(64, 2 ** 30)]
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        r = rng.integers(-1000, 1000, 64); r[lane] = INT_MIN; rows.append(r)
        r = rng.integers(-1000, 1000, 64); r[lane] = INT_MAX; rows.append(r)
        r = rng.integers(-1000, 1000, 64); r[lane] = INT_MIN; r[63 - lane] = INT_MAX; rows.append(r)
    for _ in range(16):
        rows.append(rng.integers(INT_MIN, INT_MAX + 1, 64))                       # sums that wrap
    rows.append(np.arange(64)); rows.append((np.arange(64) == 5).astype(np.int64))
    return np.array(rows, dtype=np.int64)


def wrap32(v):
    return ((np.asarray(v, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def wave_sum_i(rows):
    return wrap32(rows.sum(axis=1))


def row_shr(rows, n, ident):
    """lane i <- lane i - n of its own row of 16 lanes; `ident` where that leaves the row"""
    out = np.full_like(rows, ident)
    lane = np.arange(64)
    ok = (lane % 16) >= n
    out[:, ok] = rows[:, lane[ok] - n]
    return out


def row_shl(rows, n, ident):
    out = np.full_like(rows, ident)
    lane = np.arange(64)
    ok = (lane % 16) + n <= 15
    out[:, ok] = rows[:, lane[ok] + n]
    return out


def shfl_xor(rows, m):
    return rows[:, np.arange(64) ^ m]


@functools.lru_cache(maxsize=None)
def lane_words():
    """64 waves of 64-bit words and one replacement word per wave: wave w writes / reads lane w"""
    rng = np.random.default_rng(39)
    v = rng.integers(0, 2 ** 64, (64, 64), dtype=np.uint64)
    x = rng.integers(0, 2 ** 64, (64, 64), dtype=np.uint64)       # only column 0 is read (the wave-uniform operand)
    x[0, 0] = np.uint64(0); x[63, 0] = np.uint64(2 ** 64 - 1)
    return v, x


def writelane(v, x):
    out = v.copy()
    out[np.arange(64), np.arange(64)] = x[:, 0]
    return out


def readlane(v):
    return np.repeat(v[np.arange(64), np.arange(64)][:, None], 64, axis=1)
