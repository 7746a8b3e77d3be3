"""The device arithmetic of csrc/crowdnav_device.h against Python and numpy, op by op and EXACTLY: the roundings, the constant
divisions, the IoU, the bare-instruction helpers and the wave helpers each have one right answer, so every comparison here is
np.array_equal and there is no tolerance in this file.  References and input sets: tests/device_math_ref.py (its docstring has
the domains); tests/test_device_math_helpers.py shows on the CPU that those sets reject each plausible wrong variant.  The ops
run through cn_debug_math_n of the profiling build (one element per thread, one launch and one synchronise per call).

Exec masks.  The roundings and the IoU are called by the env kernels inside lane-divergent code (`if (i < n - 1)`, `for (k = lane;
k < R; k += 64)`), so the tie ballot of cn_round_scaled meets partial masks: they are run here at lengths 1, 63, 64, 65 and with
a ragged last wave.  The wave helpers are not: every call site of cn_wave_min_d / max_d / min_i / max_i / sum_i, of the
cn_row_shr_i scans and of cn_writelane_u64 / cn_readlane_u64 in crowdnav_kernel.hip sits in wave-uniform control flow (uniform
loops over words or blocks, `if (w0)`, `if (W <= 16)`, after the divergent loop has reconverged) of kernels launched with whole
wavefronts, one per environment -- all 64 lanes active.  cn_row_shl_i and cn_shfl_xor_d have no call site left.  They are tested
under that mask only (the entry point refuses a length that is not a multiple of 64); what a DPP reduction returns under a
partial mask is not part of their contract and is not probed."""
import ctypes as C
import functools

import numpy as np
import pytest

import device_math_ref as R

pytestmark = pytest.mark.gpu

OP = dict(round_scaled={3: 0, 2: 1}, py_round={3: 2, 2: 3}, py_round_t={3: 4, 2: 5}, np_around={3: 6, 2: 7}, np_around_t={3: 8, 2: 9},
          round_np64_t=10, round_np64=11, div={3: 12, 2: 13}, div_z=14, iou3=15, iou3_positive=16, vmin=17, vmax=18, vmax_s=19,
          vclamp=20, xorsign=21, fma_s=22, wave_min_d=30, wave_max_d=31, wave_min_i=32, wave_max_i=33, wave_sum_i=34, shfl_xor_d=35,
          row_shr={1: 40, 2: 41, 4: 42, 8: 43, 15: 44}, row_shl={1: 45, 2: 46, 4: 47, 8: 48, 15: 49}, writelane=50, readlane=51)


@functools.lru_cache(maxsize=None)
def _lib():
    import crowdnav
    L = C.CDLL(crowdnav._abi.build_timing())
    L.cn_debug_math_n.argtypes = [C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    L.cn_debug_math_n.restype = C.c_int
    return L


def _dev(op, a, b=None, c=None, d=None, e=None, py2=0, s=0.0):
    """one launch; float64 arrays travel as their bit patterns (NaNs and 64-bit words arrive untouched)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    ins = [torch.from_numpy(np.ascontiguousarray(a if v is None else v, dtype=np.float64).ravel().view(np.int64).copy()).cuda() for v in (a, b, c, d, e)]
    assert all(t.numel() == a.size for t in ins)
    out = torch.empty_like(ins[0])
    torch.cuda.synchronize()
    assert _lib().cn_debug_math_n(op, py2, float(s), *[t.data_ptr() for t in ins], out.data_ptr(), a.size, None) == 0
    return out.cpu().numpy().view(np.float64)


def _same(got, ref):
    return np.array_equal(got, ref)


def _same_bits(got, ref):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(ref, dtype=np.float64).view(np.uint64))


def _rounding_cases(nd, py2):
    """(name, op, input set name, reference function) for every rounding form at nd decimals"""
    cases = [("cn_round_scaled", OP["round_scaled"][nd], "guarded", lambda x: R.round_scaled(x, nd, py2)),
             ("cn_py_round", OP["py_round"][nd], "guarded", lambda x: R.py_round(x, nd, py2)),
             ("cn_py_round_t<true>", OP["py_round_t"][nd], "small", lambda x: R.py_round(x, nd, py2)),
             ("cn_np_around", OP["np_around"][nd], "guarded", lambda x: R.np_around(x, nd)),
             ("cn_np_around_t<true>", OP["np_around_t"][nd], "small", lambda x: R.np_around(x, nd))]
    if nd == 2:
        cases += [("cn_round_np64_2_t<false>", OP["round_np64"], "guarded", lambda x: R.round_np64(x, 2, py2)),
                  ("cn_round_np64_2_t<true>", OP["round_np64_t"], "small", lambda x: R.round_np64(x, 2, py2))]
    return cases


@pytest.mark.parametrize("py2", [0, 1])
@pytest.mark.parametrize("nd", [3, 2])
def test_roundings_equal_python_and_numpy_on_the_whole_set(nd, py2):
    """Every rounding form equals its reference in value on its whole set: ROUND_GUARDED (|x p| < 2^52) for the guarded forms,
    ROUND_SMALL (below the 2^31 guard) for the `_t<true>` forms.  (The sign of a zero result has its own test below.)"""
    sets = dict(guarded=np.array(R.round_guarded(nd)), small=np.array(R.round_small(nd)))
    assert sets["guarded"].size % 64 != 0 or sets["small"].size % 64 != 0
    refs = {}
    for name, op, which, ref in _rounding_cases(nd, py2):
        x = sets[which]
        got = _dev(op, x, py2=py2)
        want = ref(x)
        bad = np.nonzero(got != want)[0]
        print("%s nd=%d py2=%d: %d inputs, %d differ" % (name, nd, py2, x.size, bad.size))
        assert _same(got, want), (name, nd, py2, bad.size, x[bad[:5]].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        refs[name] = got
    assert (R.py_round(sets["guarded"], nd, 0) != R.py_round(sets["guarded"], nd, 1)).sum() > 0


@pytest.mark.parametrize("py2", [0, 1])
@pytest.mark.parametrize("nd", [3, 2])
def test_rounding_tie_ballot_under_partial_masks_and_single_lanes(nd, py2):
    """The exact-tie branch is taken on a wave ballot.  One tie in lane 0, in lane 63, in one lane of one wave of five, in every
    lane, in none, and two in a ragged last wave of 41 lanes -- all in one launch, each layout in wavefronts of its own -- then
    launches of 1, 63, 64 and 65 inputs that are ALL ties, so the ballot and the repair run under a partial exec mask."""
    lay = R.tie_layouts(nd)
    order = ["lane0", "lane63", "one_lane_of_one_wave", "all", "none", "two_in_the_ragged_last_wave"]
    x = np.concatenate([lay[k][0] for k in order])
    ties = np.concatenate([lay[k][1] for k in order])
    assert x.size % 64 == 41 and all(lay[k][0].size % 64 == 0 for k in order[:-1]) and ties.sum() == 1 + 1 + 1 + 192 + 0 + 2
    allt = lay["all"][0]
    for name, op, _, ref in _rounding_cases(nd, py2):
        got, want = _dev(op, x, py2=py2), ref(x)
        assert _same(got, want), (name, nd, py2, np.nonzero(got != want)[0][:8].tolist())
        for n in (1, 63, 64, 65):
            got, want = _dev(op, allt[:n], py2=py2), ref(allt[:n])
            assert _same(got, want), (name, nd, py2, n, np.nonzero(got != want)[0][:8].tolist())
    # the layouts do exercise the branch: the two Python versions part on them (on the exact ties whose even neighbour lies
    # towards zero -- about half of the exact half of the ties)
    assert (R.py_round(x, nd, 0) != R.py_round(x, nd, 1)).sum() > 0


@pytest.mark.parametrize("py2", [0, 1])
def test_unguarded_forms_are_bit_identical_to_the_guarded_ones_below_the_guard(py2):
    for nd in (3, 2):
        x = np.array(R.round_small(nd))
        pairs = [("py_round", "py_round_t"), ("np_around", "np_around_t")]
        for g, t in pairs:
            assert _same_bits(_dev(OP[g][nd], x, py2=py2), _dev(OP[t][nd], x, py2=py2)), (g, nd, py2)
    x = np.array(R.round_small(2))
    assert _same_bits(_dev(OP["round_np64"], x, py2=py2), _dev(OP["round_np64_t"], x, py2=py2))


def test_sign_of_a_zero_result():
    """Python and numpy return -0.0 for a negative x that rounds to zero (round(-0.0004, 3), np.around(-0.0004, 3), round(-0.0, 3)).
    The device returns +0.0 from every form that divides with cn_div1000 / cn_div100 -- all of them, guarded or not, below the
    guard: fma(fma(-q, P, r), 1 / P, q) with r = q = -0.0 adds the +0 of the inner fma to -0, which is +0 under round-to-nearest.
    cn_round_scaled itself keeps the sign (rint(-0.3) = -0.0).  The difference is accepted and PINNED here, not repaired: no
    consumer of a rounded value in crowdnav_kernel.hip reads the sign of a zero ("device arithmetic, op by op", goes
    through them: differences and comparisons, atan2 arguments only after a subtraction, no divisor, no bit cast, the float32 and
    float64 observation stores compared as numbers), and repairing it would add instructions to every one of the ~40 roundings of
    a step.  Everywhere else the sign of the device's result is Python's."""
    for nd in (3, 2):
        x = np.array(R.round_small(nd))
        for py2 in (0, 1):
            for name, op, _, ref in _rounding_cases(nd, py2):
                xs = x                                       # the guarded forms too: below the guard they divide the same way
                got, want = _dev(op, xs, py2=py2), ref(xs)
                assert _same(got, want)
                neg0 = (want == 0.0) & np.signbit(want)
                assert neg0.sum() > 2000 and np.signbit(xs[neg0]).all() and (xs == 0.0).sum() >= 2
                print("%s nd=%d py2=%d: %d results of -0.0 due, device gives -0.0 on %d of them" % (name, nd, py2, neg0.sum(), np.signbit(got[neg0]).sum()))
                assert np.array_equal(np.signbit(got[~neg0]), np.signbit(want[~neg0])), name      # every other sign is Python's
                if name == "cn_round_scaled":
                    assert np.signbit(got[neg0]).all(), name                                       # rint keeps it
                else:
                    assert not np.signbit(got[neg0]).any(), name                                   # the pinned difference: +0.0
    z = np.array([-0.0, 0.0, -1.0, 1.0])
    for nd in (3, 2):
        got = _dev(OP["div"][nd], z)
        assert _same(got, z / R.P10[nd]) and list(np.signbit(got)) == [False, False, True, False]  # cn_div1000(-0.0) = +0.0: the same addition


def test_constant_division_equals_the_divide():
    r = np.array(R.div_set())
    for nd in (3, 2):
        got = _dev(OP["div"][nd], r)
        assert _same(got, r / R.P10[nd]), (nd, r[got != r / R.P10[nd]][:5].tolist())
    a, b = R.divz_set()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = a / b
    got = _dev(OP["div_z"], a, b)
    assert np.isnan(want).sum() > 100 and np.isinf(want).sum() > 1000
    assert np.array_equal(got, want, equal_nan=True)
    inf = np.isinf(want)
    assert np.array_equal(np.signbit(got[inf]), np.signbit(want[inf]))


@pytest.mark.parametrize("py2", [0, 1])
def test_iou_equals_the_rational_reference_and_the_shortcut_equals_it(py2):
    ax, ay, bx, by, half = R.iou_set()
    want = R.iou3(ax, ay, bx, by, half, py2)
    got = _dev(OP["iou3"], ax, ay, bx, by, half, py2=py2)
    bad = np.nonzero(got != want)[0]
    print("cn_iou3 py2=%d: %d pairs, %d differ; %d positive, %d in the sliver" % (py2, want.size, bad.size, (want > 0).sum(),
                                                                                 ((R.iou_ratio(ax, ay, bx, by, half) < 0.00075) & (want > 0)).sum()))
    assert _same(got, want), (bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
    assert not np.signbit(got).any()
    pos = _dev(OP["iou3_positive"], ax, ay, bx, by, half, py2=py2)
    assert _same(pos, (got > 0.0).astype(np.float64)) and _same(pos, (want > 0.0).astype(np.float64))
    for n in (1, 63, 65):                                    # the ballot inside under a partial mask
        k = slice(7500, 7500 + n)
        assert _same(_dev(OP["iou3"], ax[k], ay[k], bx[k], by[k], half[k], py2=py2), want[k])


def test_bare_instruction_helpers():
    """v_min_f64 / v_max_f64 / v_fma_f64 in inline assembly and the sign transfer: values equal numpy's fmin / fmax (a quiet NaN
    in either operand returns the other), the sign of a zero equal wherever C defines it, xorsign bit for bit."""
    a, b, c = R.pair_set()
    nan_a, nan_b = np.isnan(a) & ~np.isnan(b), np.isnan(b) & ~np.isnan(a)
    assert nan_a.sum() >= 12 and nan_b.sum() >= 12
    sd = R.sign_defined(a, b)
    for op, f in ((OP["vmin"], np.fmin), (OP["vmax"], np.fmax)):
        got, want = _dev(op, a, b), f(a, b)
        assert np.array_equal(got, want, equal_nan=True)
        assert _same_bits(got[nan_a], b[nan_a]) and _same_bits(got[nan_b], a[nan_b])
        ok = sd & ~np.isnan(want)
        assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    for s in (0.12, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0):
        got, want = _dev(OP["vmax_s"], a, s=s), np.fmax(a, s)
        assert np.array_equal(got, want, equal_nan=True), s
        ok = R.sign_defined(a, np.full_like(a, s)) & ~np.isnan(want)
        assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), s
        if s == s:
            assert np.all(got[np.isnan(a)] == s)
    got, want = _dev(OP["vclamp"], a, b, c), np.fmin(np.fmax(a, b), c)
    assert np.array_equal(got, want, equal_nan=True)
    assert _same_bits(_dev(OP["xorsign"], a, b), R.xorsign(a, b))
    fa, fb = R.fma_set()
    for s in R.FMA_SCALARS:
        want = np.array([R.fma(fa[i], fb[i], s) for i in range(fa.size)])
        got = _dev(OP["fma_s"], fa, fb, s=s)
        assert _same(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), s


def test_wave_reductions_and_lane_moves():
    """Whole wavefronts, as the kernels call them: the extremum in each of the 64 lanes in turn, all lanes equal, signed zeros,
    infinities, one quiet NaN (skipped, as fmin / fmax do), INT_MIN / INT_MAX, sums that wrap; the row shifts for N = 1, 2, 4, 8,
    15 with the identities the scans use (0, -1) and one they do not; write and read of every lane 0..63."""
    d = R.wave_rows_d()
    for op, f in ((OP["wave_min_d"], np.fmin), (OP["wave_max_d"], np.fmax)):
        got = _dev(op, d).reshape(d.shape)
        want = np.repeat(f.reduce(d, axis=1)[:, None], 64, axis=1)
        assert not np.isnan(want).any() and _same(got, want), np.nonzero((got != want).any(axis=1))[0][:8].tolist()
        nz = want != 0.0
        assert np.array_equal(np.signbit(got[nz]), np.signbit(want[nz]))
    i = R.wave_rows_i()
    fi = i.astype(np.float64)
    for op, want in ((OP["wave_min_i"], i.min(axis=1)), (OP["wave_max_i"], i.max(axis=1)), (OP["wave_sum_i"], R.wave_sum_i(i))):
        got = _dev(op, fi).reshape(i.shape)
        assert _same(got, np.repeat(want[:, None], 64, axis=1).astype(np.float64)), op
    for m in (1, 2, 4, 8, 16, 32, 63):
        assert _same_bits(_dev(OP["shfl_xor_d"], d, s=m).reshape(d.shape), R.shfl_xor(d, m)), m
    for n in (1, 2, 4, 8, 15):
        for ident in (0, -1, R.INT_MIN + 5):
            assert _same(_dev(OP["row_shr"][n], fi, s=ident).reshape(i.shape), R.row_shr(i, n, ident).astype(np.float64)), (n, ident)
            assert _same(_dev(OP["row_shl"][n], fi, s=ident).reshape(i.shape), R.row_shl(i, n, ident).astype(np.float64)), (n, ident)
    v, x = R.lane_words()
    got = _dev(OP["writelane"], v.view(np.float64), x.view(np.float64)).view(np.uint64).reshape(64, 64)
    assert np.array_equal(got, R.writelane(v, x))
    got = _dev(OP["readlane"], v.view(np.float64)).view(np.uint64).reshape(64, 64)
    assert np.array_equal(got, R.readlane(v))


def test_entry_point_refuses_what_it_cannot_run():
    import torch
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = [t.data_ptr()] * 6
    L = _lib()
    assert L.cn_debug_math_n(OP["wave_sum_i"], 0, 0.0, *p, 63, None) == -2            # a partial wave for a wave helper
    assert L.cn_debug_math_n(23, 0, 0.0, *p, 64, None) == -2 and L.cn_debug_math_n(OP["vmin"], 0, 0.0, *p, 0, None) == -2
