"""CPU checks of tests/device_math_ref.py, the references and input sets of tests/test_gpu_device_math.py: the references agree
with each other where two statements of one rule exist (the builtin round and Decimal, np.around and round(np.float64)), the
Python-2.7 rule reproduces the pairs recorded from a real 2.7, the IoU reference reproduces the reference's own shapely results
under tests/golden/, and -- the point of the file -- the input sets can tell right from wrong: a float64 emulation of the device
algorithm as written equals the reference on every input, and each plausible wrong variant of it differs on at least one."""
import os

import numpy as np
import pytest

import device_math_ref as R
from conftest import GOLDEN


# ---- the device algorithms in numpy (float64, exact fma through rationals on the few lanes that need one) ------------------------
def _div_const(r, p, how):
    if how == "divide":
        return r / p
    if how == "reciprocal":
        return r * (1.0 / p)
    inv = 1.0 / p                                        # "two_fma": cn_div1000 / cn_div100 as written
    q = r * inv
    out = np.empty_like(r)
    for i in range(r.size):
        out[i] = R.fma(R.fma(-q[i], p, r[i]), inv, q[i])
    return out


def _round_scaled(x, p, py2, repair="as_written"):
    y = x * p
    r = np.rint(y)
    for i in np.nonzero(np.abs(y - r) == 0.5)[0]:
        err = R._F(float(x[i])) * R._F(p) - R._F(float(y[i]))         # fma(x, p, -y): exact, only its sign is used
        up, down = y[i] + 0.5, y[i] - 0.5
        if repair == "none":
            continue
        if repair == "swapped":
            up, down = down, up
        if err > 0: r[i] = up
        elif err < 0: r[i] = down
        elif py2: r[i] = y[i] + np.copysign(0.5, y[i])
    return r


def _py_round(x, nd, py2, repair="as_written", div="divide"):
    return _div_const(_round_scaled(x, R.P10[nd], py2, repair), R.P10[nd], div)


def _np_around(x, nd, div="divide", half_away=False):
    y = x * R.P10[nd]
    r = np.copysign(np.floor(np.abs(y) + 0.5), y) if half_away else np.rint(y)
    return _div_const(r, R.P10[nd], div)


def _round_np64(x, nd, py2, swap=False):
    """cn_round_np64_2_t: numpy's rule, the builtin's on a tie of the product under Python 2.7 (swap: the two exchanged)"""
    return _py_round(x, nd, True) if (bool(py2) != swap) else _np_around(x, nd)


def _differ(a, b):
    return int(((a != b) & ~(np.isnan(a) & np.isnan(b))).sum())


def _past_the_guard(f, x, nd):
    """The `_t<true>` form used past its guard.  In VALUE it cannot be told from the guarded form, on this set or on any: for an
    integer |r| < 2^53 the quotient r / P lies at least ulp / (2 P) from every rounding boundary, and the two-fma division is
    off the exact quotient by about 1e-16 ulp (its remainder is exact), so it rounds the same way -- 2^31 is where the
    EXHAUSTIVE check (tools/check_const_div.c) stops, not where the sequence starts to fail.  That is asserted as an equality
    so that the statement is checked; what the guard buys is the proof, and what the `<true>` forms owe is bit equality with
    the guarded ones below it (tests/test_gpu_device_math.py)."""
    big = x[np.abs(x * R.P10[nd]) >= R.GUARD]
    assert big.size > 20000 and _differ(f(big, "two_fma"), f(big, "divide")) == 0


# ---- the references against each other and against recorded results -----------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 3])
def test_two_statements_of_each_rounding_rule_agree(nd):
    x = R.round_guarded(nd)
    a, b = R.py3_round(x, nd), R.py3_round_decimal(x, nd)
    assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))
    a, b = R.np_around(x, nd), R.np64_round(x, nd)
    assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))
    # the two Python versions part on exact ties only, and the set has them
    d = R.py3_round(x, nd) != R.py27_round(x, nd)
    assert d.sum() > 0 and np.all(np.abs(x[d] * R.P10[nd] - np.rint(x[d] * R.P10[nd])) == 0.5)
    z = R.round_scaled(x, nd, 0)
    assert np.array_equal(z, np.rint(z)) and np.array_equal(z / R.P10[nd], R.py3_round(x, nd))


def test_python27_rule_reproduces_the_recorded_pairs():
    """the pairs tests/test_oracle_golden.py records from the reference's Python 2.7, and the same inputs under Python 3"""
    for x, nd, want in ((0.0625, 3, 0.063), (-0.0625, 3, -0.063), (0.125, 2, 0.13), (0.3125, 3, 0.313), (2.675, 2, 2.67),
                        (0.0624999999, 3, 0.062), (-0.375, 2, -0.38), (1.0005, 3, 1.0), (0.625, 2, 0.63)):
        assert R.py27_round([x], nd)[0] == want and R.round_np64([x], nd, 1)[0] == want, (x, nd)
    for x, nd, want in ((0.0625, 3, 0.062), (-0.0625, 3, -0.062), (0.125, 2, 0.12), (0.3125, 3, 0.312), (2.675, 2, 2.67), (0.625, 2, 0.62)):
        assert R.py3_round([x], nd)[0] == want, (x, nd)
        # numpy rounds the float64 PRODUCT: 2.675 x 100 is 267.5 in float64 although 2.675 lies below the tie
        assert R.round_np64([x], nd, 0)[0] == (2.68 if x == 2.675 else want), (x, nd)
    for f in (R.py3_round, R.py27_round, R.np_around):                       # a negative value that rounds to zero keeps its sign
        assert np.signbit(f([-0.0001, -0.0], 3)).all() and not np.signbit(f([0.0001, 0.0], 3)).any()


def test_iou_reference_reproduces_the_recorded_shapely_results():
    g = np.load(os.path.join(GOLDEN, "func.npz"))
    p1, p2, s = g["iou_p1"], g["iou_p2"], g["iou_s"]
    got = R.iou3(p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1], s, 0)
    assert np.array_equal(got, g["iou_out"]) and np.array_equal(got > 0.0, g["assoc_out"].astype(bool))
    assert R.iou3([0.0], [0.0], [0.05], [0.0], [0.0505], 0)[0] == 0.338


def test_iou_set_covers_its_cases():
    ax, ay, bx, by, half = R.iou_set()
    t = R.iou_ratio(ax, ay, bx, by, half)
    assert set(np.unique(half)) == set(R.HALVES)
    for h in R.HALVES:
        th = t[half == h]
        assert (th == 0.0).sum() > 100 and (th == 1.0).sum() >= 200 and ((th > 0.0003) & (th < 0.0005)).sum() > 500
        assert ((th > 0.0005) & (th < 0.00075)).sum() > 500 and ((th > 0.00075) & (th < 0.0012)).sum() > 500 and (th > 0.01).sum() > 500
    touch = np.array([R.iou_terms(*v)[0] == 0 and abs(abs(v[0] - v[2]) - 2 * v[4]) < 1e-12 for v in zip(ax, ay, bx, by, half)])
    assert touch.sum() > 100


# ---- the sets tell right from wrong ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("py2", [0, 1])
@pytest.mark.parametrize("nd", [2, 3])
def test_py_round_as_written_equals_python_and_every_wrong_variant_differs(nd, py2):
    x = np.array(R.round_guarded(nd))
    ref = R.py_round(x, nd, py2)
    assert _differ(_py_round(x, nd, py2), ref) == 0
    assert np.array_equal(_round_scaled(x, R.P10[nd], py2), R.round_scaled(x, nd, py2))
    assert _differ(_py_round(x, nd, py2, repair="none"), ref) > 0              # rint(x p) / p
    assert _differ(_py_round(x, nd, py2, repair="swapped"), ref) > 0           # the err signs exchanged
    assert _differ(_py_round(x, nd, 1 - py2), ref) > 0                         # half away for half even and the reverse
    assert _differ(_py_round(x, nd, py2, div="reciprocal"), ref) > 0           # r (1 / p)
    s = np.array(R.round_small(nd))
    assert _differ(_py_round(s, nd, py2, div="two_fma"), R.py_round(s, nd, py2)) == 0    # the <true> form inside its domain ...
    _past_the_guard(lambda v, div: _py_round(v, nd, py2, div=div), x, nd)


@pytest.mark.parametrize("nd", [2, 3])
def test_np_around_as_written_equals_numpy_and_every_wrong_variant_differs(nd):
    x = np.array(R.round_guarded(nd))
    ref = R.np_around(x, nd)
    assert _differ(_np_around(x, nd), ref) == 0
    assert _differ(_py_round(x, nd, 0), ref) > 0                               # Python's tie repair where numpy has none
    assert _differ(_np_around(x, nd, half_away=True), ref) > 0
    assert _differ(_np_around(x, nd, div="reciprocal"), ref) > 0
    s = np.array(R.round_small(nd))
    assert _differ(_np_around(s, nd, div="two_fma"), R.np_around(s, nd)) == 0
    _past_the_guard(lambda v, div: _np_around(v, nd, div=div), x, nd)


@pytest.mark.parametrize("py2", [0, 1])
def test_round_np64_as_written_equals_its_reference_and_the_swapped_rule_differs(py2):
    x = np.array(R.round_guarded(2))
    ref = R.round_np64(x, 2, py2)
    assert _differ(_round_np64(x, 2, py2), ref) == 0
    assert _differ(_round_np64(x, 2, py2, swap=True), ref) > 0
    assert _differ(_np_around(x, 2, div="reciprocal"), ref) > 0


def test_constant_division_set_rejects_the_bare_reciprocal():
    r = R.div_set()
    for p in (1000.0, 100.0):
        assert _differ(r * (1.0 / p), r / p) > 0
        assert _differ(r * (1.0 / p) * (1.0 + 2.0 ** -52), r / p) > 0
    k = r[::9973]
    assert _differ(_div_const(k, 1000.0, "two_fma"), k / 1000.0) == 0 and _differ(_div_const(k, 100.0, "two_fma"), k / 100.0) == 0


def _iou_positive(ax, ay, bx, by, half, py2, cut=0.00075, ge=False):
    """cn_iou3_positive in float64 as written (cut, ge: the shortcut's constant and comparison)"""
    axp, axm, ayp, aym = ax + half, ax - half, ay + half, ay - half
    bxp, bxm, byp, bym = bx + half, bx - half, by + half, by - half
    ix = np.minimum(axp, bxp) - np.maximum(axm, bxm)
    iy = np.minimum(ayp, byp) - np.maximum(aym, bym)
    ov = (ix > 0.0) & (iy > 0.0)
    inter = ix * iy
    uni = (axp - axm) * (ayp - aym) + (bxp - bxm) * (byp - bym) - inter
    short = (inter >= cut * uni) if ge else (inter > cut * uni)
    with np.errstate(invalid="ignore", divide="ignore"):
        exact = R.py_round(np.where(ov, inter / uni, 0.0), 3, py2) > 0.0
    return ov & (short | exact), np.where(ov, inter / uni, 0.0)


@pytest.mark.parametrize("py2", [0, 1])
def test_iou_as_written_equals_the_rational_reference_and_the_wrong_shortcuts_differ(py2):
    """The float64 quotient of the device equals the once-rounded exact quotient closely enough that their three-decimal
    roundings agree on the whole set, and the shortcut as written gives the reference's predicate.  A shortcut whose cut lies
    BELOW the tie (0.0004) or that skips the exact path for the sliver (0.00075 as the whole test) is told apart by the dense
    sweep.  Two variants are not, on this or on any set, because they are the same predicate as the one written:
    - `>=` for `>` at 0.00075: equality means a quotient within an ulp of 0.00075, which rounds to 0.001 like all above it;
    - 0.0005 for 0.00075 with `>`: the float64 0.0005 lies ABOVE the decimal tie, and inter > fl(0.0005 uni) puts inter at
      least half an ulp above 0.0005 uni, so fl(inter / uni) >= 0.0005 and it rounds to 0.001 under either Python.
    With `>=` at 0.0005 the shortcut errs only where inter EQUALS fl(0.0005 uni) to the last bit and that product was rounded
    down; the sweep (steps of 3e-7 in the ratio) has no such pair, and within an ulp of the tie the once-rounded exact quotient
    of the reference and the float64 quotient of the reference's shapely need not agree either, so no such pair is planted.
    The three are asserted EQUAL to the reference here so that the statement above is checked, not assumed."""
    ax, ay, bx, by, half = R.iou_set()
    ref = R.iou3(ax, ay, bx, by, half, py2)
    got, quo = _iou_positive(ax, ay, bx, by, half, py2)
    assert np.array_equal(R.py_round(quo, 3, py2), ref)
    assert np.array_equal(got, ref > 0.0)
    assert (_iou_positive(ax, ay, bx, by, half, py2, cut=0.0004)[0] != (ref > 0.0)).sum() > 0
    axp, axm, bxp, bxm = ax + half, ax - half, bx + half, bx - half
    ayp, aym, byp, bym = ay + half, ay - half, by + half, by - half
    ix, iy = np.minimum(axp, bxp) - np.maximum(axm, bxm), np.minimum(ayp, byp) - np.maximum(aym, bym)
    uni = (axp - axm) * (ayp - aym) + (bxp - bxm) * (byp - bym) - ix * iy
    only_shortcut = (ix > 0.0) & (iy > 0.0) & (ix * iy > 0.00075 * uni)                   # no exact path behind the shortcut
    assert (only_shortcut != (ref > 0.0)).sum() > 0
    for cut, ge in ((0.00075, True), (0.0005, False), (0.0005, True)):
        assert np.array_equal(_iou_positive(ax, ay, bx, by, half, py2, cut=cut, ge=ge)[0], ref > 0.0)


# ---- bare-instruction and wave references ----------------------------------------------------------------------------------------
def test_fma_reference_rounds_once_and_keeps_ieee_zeros():
    assert R.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104            # a b + c in float64 would give 0
    assert R.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    z = [R.fma(0.0, 1.0, 0.0), R.fma(-0.0, 1.0, -0.0), R.fma(-0.0, 1.0, 0.0), R.fma(1.0, 1.0, -1.0), R.fma(0.0, -2.0, -0.0)]
    assert z == [0.0] * 5 and [bool(np.signbit(v)) for v in z] == [False, True, False, False, True]
    a, b = R.fma_set()
    naive = sum(int(R.fma(a[i], b[i], s) != a[i] * b[i] + s) for i in range(a.size) for s in R.FMA_SCALARS[:2])
    assert naive > 0                                                                  # the set tells a fused from an unfused multiply-add


def test_wave_references_on_known_rows():
    d, i = R.wave_rows_d(), R.wave_rows_i()
    assert np.array_equal(np.fmin.reduce(d[:64], axis=1), -100.0 - np.arange(64)) and np.array_equal(np.fmax.reduce(d[:64], axis=1), 100.0 + np.arange(64))
    assert np.isnan(d).any(axis=1).sum() == 8 and not np.isnan(np.fmin.reduce(d, axis=1)).any() and not np.isnan(np.fmax.reduce(d, axis=1)).any()
    assert np.array_equal(i[:64].min(axis=1), -5000 - np.arange(64)) and (i == R.INT_MIN).any() and (i == R.INT_MAX).any()
    assert (R.wave_sum_i(i) != i.sum(axis=1)).sum() >= 8 and R.wave_sum_i(np.full((1, 64), 2 ** 30))[0] == 0
    lanes = np.arange(64)[None, :]
    assert list(R.row_shr(lanes, 1, -1)[0][:18]) == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, -1, 16]
    assert list(R.row_shl(lanes, 15, -7)[0][:17]) == [15] + [-7] * 15 + [31]
    assert list(R.row_shr(lanes, 15, 9)[0][14:17]) == [9, 0, 9] and R.row_shr(lanes, 15, 9)[0][31] == 16
    assert list(R.shfl_xor(lanes, 32)[0][:2]) == [32, 33]
    v, x = R.lane_words()
    w = R.writelane(v, x)
    assert (w != v).sum() == 64 and all(w[k, k] == x[k, 0] for k in range(64)) and np.array_equal(R.readlane(v)[:, 7], np.diag(v))
