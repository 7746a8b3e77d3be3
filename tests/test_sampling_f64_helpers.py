"""CPU checks of tests/sampling_f64.py, the statement the GPU tests hold td3_prep_kernel's replay indices and target-policy noise
to: the numpy generator equals a pure-Python-integer one, the statement is a sound sampler (uniform, uncorrelated, normal), and
every wrong variant differs from it on the GPU test's own plan -- so a pass there rules each of them out."""
import math

import numpy as np
import pytest

import sampling_f64 as S

MASK64 = (1 << 64) - 1


def _mix64_int(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _hash_int(seed, counter, m):
    return _mix64_int(_mix64_int(seed ^ _mix64_int(counter & MASK64)) ^ (m & 0xFFFFFFFF))


def _index_int(seed, counter, m, size):
    return _hash_int(seed, counter, m) % max(size, 1)


@pytest.mark.parametrize("seed", (0, 1, MASK64, 0x6A09E667F3BCC908, 1 << 63))
@pytest.mark.parametrize("counter", (0, 1, 2, 63, (1 << 32) + 5, MASK64))
def test_numpy_generator_equals_python_integers(seed, counter):
    rows = list(range(5)) + [127, 128, 4095, (1 << 31) + 3]
    for size in (1, 2, 37, 5003, (1 << 20) - 1, 1_000_000, (1 << 24) + 1, (1 << 40) + 17, 0, -1, -(1 << 63)):
        want = [_index_int(seed, counter, m, size) for m in rows]
        got = list(S.indices(seed, counter, None, size, rows=rows))
        assert got == want, (seed, counter, size)
    h = S.noise_hash(seed, counter, None, rows=rows)
    want_h = [_hash_int(seed, counter ^ S.NOISE_XOR, m) for m in rows]
    assert [int(x) for x in h] == want_h
    # the noise: u1, u2 from the integers, the float32 angle from Python's float32 rounding of the product
    noise, _ = S.target_noise(seed, counter, 4096, 1.0, 100.0)
    for i, m in enumerate(rows[:-1]):
        hm = want_h[i]
        u1 = ((hm >> 40) + 1) / 2.0 ** 24
        u2 = ((hm >> 8) & 0xFFFFFF) / 2.0 ** 24
        a = float(np.float32(np.float32(u2) * np.float32(6.28318530718)))
        r = math.sqrt(-2.0 * math.log(u1))
        assert abs(noise[m, 0] - r * math.cos(a)) <= 1e-15 * r and abs(noise[m, 1] - r * math.sin(a)) <= 1e-15 * r   # (libm vs numpy)


def test_degenerate_sizes_are_taken_as_one():
    for size in (0, -1, -(1 << 63)):
        assert (S.indices(7, 3, 64, size) == 0).all()


def _chi2_ok(counts, expected):
    df = counts.size - 1
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    return chi2 < df + 6 * math.sqrt(2 * df), chi2


@pytest.mark.parametrize("size", (37, 5003, (1 << 20) - 1))
def test_indices_are_uniform(size):
    idx = np.concatenate([S.indices(11, c, 4096, size) for c in range(64)])       # 2^18 draws
    assert idx.min() >= 0 and idx.max() < size
    bins = min(size, 4096)
    counts = np.bincount(idx * bins // size, minlength=bins).astype(np.float64)
    expected = np.bincount(np.arange(size) * bins // size, minlength=bins) * (idx.size / size)
    ok, chi2 = _chi2_ok(counts, expected)
    assert ok, (size, chi2, bins)
    if size > 4096:          # the low bits as well: a remainder that kept only the high word would pass the coarse bins
        ok, chi2 = _chi2_ok(np.bincount(idx % 256, minlength=256).astype(np.float64),
                            np.bincount(np.arange(size) % 256, minlength=256) * (idx.size / size))
        assert ok, (size, chi2)


def _corr(x, y):
    x = x - x.mean()
    y = y - y.mean()
    return float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum()))


def test_no_correlation_between_rows_counters_or_noise_columns():
    size = 1_000_000
    u = np.stack([S.indices(5, c, 4096, size) for c in range(65)]).astype(np.float64) / size      # [counter, row]
    n = u[:, :-1].size
    lim = 5.0 / math.sqrt(n)
    assert abs(_corr(u[:, :-1].ravel(), u[:, 1:].ravel())) < lim            # neighbouring rows
    assert abs(_corr(u[:-1].ravel(), u[1:].ravel())) < lim                  # consecutive updates, same row
    z = np.concatenate([S.target_noise(5, c, 4096, 1.0, 100.0)[0] for c in range(64)])
    lim = 5.0 / math.sqrt(z.shape[0])
    assert abs(_corr(z[:, 0], z[:, 1])) < lim
    assert abs(_corr(z[:, 0] ** 2, z[:, 1] ** 2)) < 2 * lim                  # independent, not only uncorrelated
    assert abs(_corr(z[:-1, 0], z[1:, 0])) < lim


def test_box_muller_moments():
    z = np.concatenate([S.target_noise(9, c, 4096, 1.0, 100.0)[0] for c in range(64)]).ravel()     # 2^19 values
    n = z.size
    assert abs(z.mean()) < 5 / math.sqrt(n)
    assert abs((z ** 2).mean() - 1) < 5 * math.sqrt(2 / n)
    assert abs((z ** 4).mean() - 3) < 5 * math.sqrt(96 / n)
    assert abs((z ** 3).mean()) < 5 * math.sqrt(15 / n)
    assert np.abs(z).max() <= S.r_max()


def test_noise_zeros_and_allowance():
    _, b = S.target_noise(1, 0, 256, 0.2, 0.5)
    n0, b0 = S.target_noise(1, 0, 256, 0.0, 0.5)
    assert (n0 == 0).all() and (b0 == 0).all()
    n0, _ = S.target_noise(1, 0, 256, 0.25, 0.0)
    assert (n0 == 0).all()
    z, _ = S.target_noise(1, 0, 256, 1.0, 100.0)
    assert np.allclose(b, S.E_NOISE * S.SLACK * float(np.float32(0.2)) * np.abs(z))
    assert S.E_NOISE == 8 * S.U


# ---- the wrong variants, on the GPU test's plan --------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.INDEX_VARIANTS)
def test_every_index_variant_differs_on_the_gpu_plan(variant):
    """On every (batch, seed) handle of the GPU index test the variant's indices differ from the statement's at some update; with
    129 and 4096 rows, at every live size above 2 (and from 2 on when the variant changes the divisor)."""
    for B in S.BATCHES:
        for seed in S.INDEX_SEEDS:
            differ = []
            for k, size in enumerate(S.index_plan()):
                a = S.indices(seed, k, B, size)
                b = S.indices(seed, k, B, size, variant=variant, capacity=S.CAPACITY)
                differ.append(bool((a != b).any()))
                if B > 1 and S.live(size) > 2:
                    assert differ[-1], (variant, B, seed, k, size)
            assert any(differ), (variant, B, seed)


def _worst_ratio(got, want, bound):
    d = np.abs(got - want)
    return float(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0)).max())


@pytest.mark.parametrize("variant", S.NOISE_VARIANTS)
def test_every_noise_variant_breaks_the_allowance_on_the_gpu_plan(variant):
    """Twice the allowance: a device result within it of the statement is then beyond it from the variant."""
    worst = 0.0
    for seed in S.NOISE_SEEDS[:1]:
        for std, clip in S.NOISE_SETTINGS:
            for c in range(4):
                want, bound = S.target_noise(seed, c, S.NOISE_B, std, clip)
                bad, _ = S.target_noise(seed, c, S.NOISE_B, std, clip, variant=variant)
                worst = max(worst, _worst_ratio(bad, want, bound))
    assert worst > 2.0, (variant, worst)


def test_the_statement_is_within_its_own_allowance_of_itself():
    for std, clip in S.NOISE_SETTINGS:
        want, bound = S.target_noise(3, 0, 512, std, clip)
        assert _worst_ratio(want, want, bound) == 0.0


# ---- the searched seeds --------------------------------------------------------------------------------------------------
def test_extreme_seeds_place_the_extremes():
    found = S.find_extreme_seeds(B=S.NOISE_B, counters=S.NOISE_UPDATES)
    assert set(found) == set(S.EXTREMES)
    for name, (seed, c, m) in found.items():
        assert 0 <= c < S.NOISE_UPDATES and 0 <= m < S.NOISE_B
        shift, val = S.EXTREMES[name]
        h = _hash_int(seed, c ^ S.NOISE_XOR, m)
        assert (h >> shift) & 0xFFFFFF == val, name
        z, b = S.target_noise(seed, c, m + 1, 1.0, 100.0)
        if name == "u1_min":
            assert abs(math.hypot(*z[m]) - S.r_max()) < 1e-12
        if name == "u1_one":
            assert (z[m] == 0).all() and (b[m] == 0).all()
        if name == "u2_zero":
            assert z[m, 1] == 0 and b[m, 1] == 0 and z[m, 0] > 0
        if name in ("u2_quarter", "u2_three_quarter"):
            assert 0 < abs(z[m, 0]) < 1e-6 * math.hypot(*z[m])
        if name == "u2_half":
            assert 0 < abs(z[m, 1]) < 1e-6 * math.hypot(*z[m])


# ---- the key the learner shares with the exploration noise ----------------------------------------------------------------
def test_exploration_noise_narrows_the_replay_index():
    """DESIGN.md's figure: with the trainer's ring of 10^6 rows, the exploration noise of environment row m under (seed, c) leaves
    batch row m of update c among 65 536 candidate ring rows (the hash's bits 0..7 and 32..39 are the ones the noise does not
    read)."""
    size = 1_000_000
    for seed, c, m in ((1, 1, 0), (0xD1B54A32D192ED03, 17, 100)):
        cand = S.index_window(seed, c, m, size)
        assert int(S.indices(seed, c, m + 1, size)[m]) in cand
        assert len(cand) == 65536
